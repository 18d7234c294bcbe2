"""Float64 references that carry a per-element error bound, for the bf16 / fp16 kernel goldens.

Shared by tests/test_bound_ref_cpu.py (CPU tier: the bound is sound for fp32 emulations in
several accumulation orders, and rejects single-element damage) and tests/test_hip_kernels.py
(the kernels on the device). Imported the way tests/int8_ref.py is.

A quantity is a pair ``(v, e)`` of float64 tensors: ``v`` the reference value, ``e`` a bound on
``|kernel - v|`` at that element. ``e`` is derived from the arithmetic below and never from
what a kernel returns. ``e`` may be ``None`` for an exact input (zero everywhere).

Linear stage (conv, depthwise, matvec; bias, per-image bias and residual as ``extras``), n
accumulated products per output, ``op`` linear in its first argument:

    v' = op(v, w) + sum(extras)
    e' = op(e, |w|) + sum(e of extras) + 2 (n + 4) 2^-24 (op(|v| + e, |w|) + sum(|extras|))

The second term is the gamma_n bound of an fp32 sum of n products in ANY order (MFMA trees,
split-K partials, per-tap chains), doubled for an accumulator that truncates where IEEE
rounds; "+ 4" covers the additions of bias, per-image bias and residual and the activation's
input. The magnitudes use ``|v| + e``: the kernel's operands are within e of v.

Activations (ReLU, ReLU6, clamp) are monotone and 1-Lipschitz: v is clamped, and e becomes
max(act(v + e) - act(v), act(v) - act(v - e)): never more than e, and zero where the whole
interval is clamped (a value at least e below zero is exactly zero after a ReLU).

Rounding stage (``round_stage``; bf16: 8 significant bits, fp16: 11, each with its subnormal
spacing, round to nearest even). Rounding is monotone, so a kernel value x in [v - e, v + e]
rounds into [rnd(v - e), rnd(v + e)]:

    v_r = rnd(v),   e_r = max(rnd(v + e) - v_r, v_r - rnd(v - e))

That is zero exactly where no rounding midpoint of the format lies within e of v (the kernel's
rounded value then equals v_r: the error is reset), and at most e + ulp elsewhere (a flip is
possible). It is the tightest bound that holds for every x in the interval; the plain
``e + ulp(v)`` is not one when v - e and v + e lie in different binades.
"""
from __future__ import annotations

from typing import Callable, Optional, Sequence, Tuple

import torch

U32 = 2.0 ** -24
FORMATS = {"bf16": (8, -126), "fp16": (11, -14)}  # significant bits, smallest normal exponent
TORCH_DTYPE = {"bf16": torch.bfloat16, "fp16": torch.float16}

Pair = Tuple[torch.Tensor, Optional[torch.Tensor]]


def ulp(v: torch.Tensor, fmt: str) -> torch.Tensor:
    """Spacing of the format's numbers at |v| (the subnormal spacing below the smallest normal)."""
    p, emin = FORMATS[fmt]
    ex = torch.frexp(v.double().abs())[1].double() - 1.0  # floor(log2 |v|); 0 for v == 0
    ex = torch.where(v == 0, torch.full_like(ex, float(emin)), ex).clamp_min(float(emin))
    return torch.exp2(ex - (p - 1))


def rnd(v: torch.Tensor, fmt: str) -> torch.Tensor:
    """float64 -> nearest number of the format, ties to even, in ONE rounding (a cast through
    fp32 would round twice). The quotient by the spacing is exact (a power of two)."""
    v = v.double()
    q = ulp(v, fmt)
    return torch.round(v / q) * q  # torch.round: half to even


def round_stage(v: torch.Tensor, e: Optional[torch.Tensor], fmt: str) -> Pair:
    v = v.double()
    vr = rnd(v, fmt)
    if e is None:
        return vr, None
    er = torch.maximum(rnd(v + e, fmt) - vr, vr - rnd(v - e, fmt))
    return vr, er


def flip_share(e: Optional[torch.Tensor]) -> float:
    """Share of the elements of a rounded pair at which a flip was possible (e_r > 0)."""
    return 0.0 if e is None else (e > 0).double().mean().item()


def linear(op: Callable[[torch.Tensor, torch.Tensor], torch.Tensor], x: Pair, w: torch.Tensor, n: int,
           extras: Sequence[Pair] = ()) -> Pair:
    """``op(x, w)`` must be linear in x and in w (no bias inside). ``extras`` are pairs that
    broadcast against the result and are added to it (bias, per-image bias, residual)."""
    v, e = x
    v, w = v.double(), w.double()
    out = op(v, w)
    mag = op(v.abs() if e is None else v.abs() + e, w.abs())
    err = torch.zeros_like(out) if e is None else op(e.double(), w.abs())
    for xv, xe in extras:
        xv = xv.double()
        out = out + xv
        mag = mag + xv.abs()
        if xe is not None:
            err = err + xe
            mag = mag + xe
    return out, err + 2.0 * (n + 4) * U32 * mag


def act(x: Pair, name: Optional[str]) -> Pair:
    v, e = x
    if name is None:
        return v, e
    hi = {"relu": None, "relu6": 6.0, "unit": 1.0}[name]
    va = v.clamp(0.0, hi)
    if e is None:
        return va, None
    return va, torch.maximum((v + e).clamp(0.0, hi) - va, va - (v - e).clamp(0.0, hi))


def assert_within(got: torch.Tensor, v: torch.Tensor, e: Optional[torch.Tensor], what: str) -> float:
    """``|got - v| <= e`` at EVERY element (nothing sampled or skipped; a non-finite ``got``
    fails). Returns max |got - v| / e (0 / 0 counts as 0, x / 0 as inf). A reference that is
    not finite, or a bound that is NaN, infinite or negative, is an error of the test:
    ``d > e`` is false against a NaN or an infinity, and such an element would pass whatever
    the kernel wrote."""
    assert got.shape == v.shape, (what, tuple(got.shape), tuple(v.shape))
    got = got.detach().double().cpu()
    e = torch.zeros_like(v) if e is None else e
    assert e.shape == v.shape, (what, tuple(e.shape), tuple(v.shape))
    assert bool(torch.isfinite(v).all()), f"{what}: the reference v is not finite"
    assert bool(torch.isfinite(e).all()) and bool((e >= 0).all()), f"{what}: the bound e is not finite or negative"
    d = (got - v).abs()
    d = torch.where(torch.isfinite(got), d, torch.full_like(d, float("inf")))
    bad = d > e
    ratio = torch.where(d == 0, torch.zeros_like(d), d / e)  # d > 0, e == 0: inf
    worst = float(ratio.max()) if ratio.numel() else 0.0
    if bool(bad.any()):
        flat = int(torch.where(bad, ratio, torch.full_like(ratio, -1.0)).argmax())
        idx = tuple(int(i) for i in torch.unravel_index(torch.tensor(flat), v.shape))
        raise AssertionError(
            f"{what}: {int(bad.sum())} of {bad.numel()} elements outside their bound; worst at {idx}: "
            f"got {got[idx].item()!r}, v {v[idx].item()!r}, e {e[idx].item()!r}; max |got - v| / e = {worst:.4g}")
    return worst


def violations(got: torch.Tensor, v: torch.Tensor, e: Optional[torch.Tensor]) -> torch.Tensor:
    """The mask ``|got - v| > e`` (for the tests of the bound itself)."""
    e = torch.zeros_like(v) if e is None else e
    return (got.detach().double().cpu() - v).abs() > e
