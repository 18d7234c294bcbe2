"""Exact references, comparators and the teacher-forced plan walker of the int8 tests.

Shared by tests/test_quant_cpu.py (CPU tier: the oracle and the comparator themselves),
tests/test_int8_plan.py (every step and every kernel variant of a ``HipDeepLabInt8`` plan)
and the headline test in tests/test_hip_kernels.py (the committed plan, picks only).

Every reference here is float64 arithmetic on integer codes: the int32 accumulators are
exact (|acc| < 2^53), the affine epilogue ``acc * s_in * s_w + b (+ img_bias) (+ res *
s_res)`` is evaluated once in float64, and requantisation is round-half-even with a clamp
to +-127. A kernel's fp32 epilogue differs from that only at rounding ties.
"""
from __future__ import annotations

from typing import Callable, Dict, List, Optional

import torch
import torch.nn.functional as F

import chip_poison as CP

MAX_STEP = 1        # a code may be one requantisation step off ...
MAX_SHARE = 1e-3    # ... on at most this share of a tensor's codes
MAX_SATURATED = 1e-2


# ---------------------------------------------------------------- comparators
def code_mismatch(got: torch.Tensor, ref: torch.Tensor):
    """(share of codes that differ, largest difference in steps)."""
    assert got.shape == ref.shape, (tuple(got.shape), tuple(ref.shape))
    d = (got.to(torch.int32) - ref.to(torch.int32)).abs()
    return int((d > 0).sum()) / d.numel(), int(d.max())


def assert_codes_close(got: torch.Tensor, ref: torch.Tensor, what: str,
                       max_share: float = MAX_SHARE, max_step: int = MAX_STEP):
    """int8 codes against exact reference codes: at most ``max_step`` off, on at most
    ``max_share`` of the codes. Returns (share, max step) for reports."""
    share, mx = code_mismatch(got, ref)
    assert mx <= max_step and share <= max_share, \
        f"{what}: {share:.3e} of the codes differ from the exact reference, by up to {mx} steps"
    return share, mx


def assert_bf16_close(got: torch.Tensor, ref: torch.Tensor, what: str):
    """bf16 output of an exact fp32 value: one bf16 rounding (relative 2^-9) with a factor
    of two of slack, elementwise."""
    got, ref = got.double(), ref.double()
    assert got.shape == ref.shape, (tuple(got.shape), tuple(ref.shape))
    assert bool(torch.isfinite(got).all()), f"{what}: output holds non-finite values"
    excess = (got - ref).abs() - (2.0 ** -8 * ref.abs() + 1e-6)
    assert float(excess.max()) <= 0.0, \
        f"{what}: {(excess > 0).double().mean().item():.3e} of the values miss the bf16 bound, " \
        f"worst excess {float(excess.max()):.3e}"


def saturated_share(codes: torch.Tensor) -> float:
    return (codes.abs() >= 127).double().mean().item()


# ---------------------------------------------------------------- exact references
def exact_conv(x_codes: torch.Tensor, wq: torch.Tensor, sw: torch.Tensor, b: torch.Tensor,
               s_in: float, *, stride: int = 1, dil: int = 1, res_codes=None, s_res: float = 0.0,
               img_bias=None, act: Optional[str] = None) -> torch.Tensor:
    """float64 value of one int8 conv before requantisation. x_codes NCHW integer-valued,
    wq [Cout, Cin, k, k] integer-valued, sw / b per output channel, img_bias [B, Cout]."""
    dev = x_codes.device
    k = wq.shape[-1]
    if k == 1:
        acc = torch.einsum("bchw,oc->bohw", x_codes.double()[:, :, ::stride, ::stride],
                           wq[:, :, 0, 0].double().to(dev))
    else:
        acc = F.conv2d(x_codes.double(), wq.double().to(dev), None, stride, dil * (k // 2), dil)
    v = acc * (s_in * sw.double().to(dev)).view(1, -1, 1, 1) + b.double().to(dev).view(1, -1, 1, 1)
    if img_bias is not None:
        v = v + img_bias.double().to(dev)[:, :, None, None]
    if res_codes is not None:
        v = v + res_codes.double() * s_res
    if act == "relu":
        v = torch.relu(v)
    elif act == "relu6":
        v = torch.clamp(v, 0.0, 6.0)
    else:
        assert act is None, act
    return v


def requant(v: torch.Tensor, s_out: float, lo: int = -127) -> torch.Tensor:
    return torch.clamp(torch.round(v / s_out), lo, 127).to(torch.int32)


def stem_pixel_table() -> torch.Tensor:
    """The 256 normalised pixel values as the stem kernels compute them: ONE rounding,
    fp32(p * fp32(1 / 127.5) - 1), a fused multiply-add (``reference_ops.preprocess`` rounds
    the product first: 158 of the 256 values are then one fp32 ulp away)."""
    c = torch.tensor(1.0 / 127.5, dtype=torch.float32).double()
    return (torch.arange(256, dtype=torch.float64) * c - 1.0).float()  # exact in float64


def letterbox_pixels(frames: torch.Tensor, lut_x, lut_y, table: torch.Tensor) -> torch.Tensor:
    """uint8 BGR frames -> (N, 3, H, W) fp32 model input through the letterbox LUTs, as
    ``reference_ops.preprocess`` gathers it, normalised by ``table``."""
    dev = frames.device
    lx = torch.as_tensor(lut_x, device=dev).long()
    ly = torch.as_tensor(lut_y, device=dev).long()
    g = frames[:, ly.clamp(min=0)][:, :, lx.clamp(min=0)]
    g = g * ((ly >= 0)[None, :, None, None] & (lx >= 0)[None, None, :, None])
    return table.to(dev)[g.flip(-1).long()].permute(0, 3, 1, 2).contiguous()


def stem_ref_values(x: torch.Tensor, w: torch.Tensor, b: torch.Tensor, stride: int,
                    bf16_operands: bool) -> torch.Tensor:
    """The fused stem conv on normalised pixels ``x`` (N, 3, H, W) before its activation:
    float64 accumulation of fp32 operands (the per-lane kernel) or of operands rounded to
    bf16 (the MFMA kernels), fp32 bias. w [Cout, 3, k, k]."""
    if bf16_operands:
        w, x = w.to(torch.bfloat16).float(), x.to(torch.bfloat16).float()
    k = w.shape[-1]
    OH = (x.shape[2] + 2 * (k // 2) - k) // stride + 1
    OW = (x.shape[3] + 2 * (k // 2) - k) // stride + 1
    wm = w.reshape(w.shape[0], -1).double().to(x.device)
    outs = []
    for i in range(x.shape[0]):  # one image at a time: the float64 im2col of 1025^2 is 0.3 GB
        cols = F.unfold(x[i:i + 1].double(), k, padding=k // 2, stride=stride)[0]
        outs.append((wm @ cols + b.double().to(x.device)[:, None]).view(-1, OH, OW))
    return torch.stack(outs)


def stem_ref_codes(x: torch.Tensor, layer, s_out: float, bf16_operands: bool) -> torch.Tensor:
    """``stem_ref_values`` of a folded ConvBNAct stem, ReLU, requantised."""
    w, b = layer.fold()
    return requant(torch.relu(stem_ref_values(x, w, b, layer.stride, bf16_operands)), s_out)


# ---------------------------------------------------------------- the plan walker
def _nchw(t: torch.Tensor) -> torch.Tensor:
    return t.permute(0, 3, 1, 2)


def plan_steps(hm) -> List[tuple]:
    """The steps of a ``HipDeepLabInt8`` plan in op order as (kind, output buffer, spec):
    mirrors ``HipDeepLabInt8._plan`` (the walker asserts the op count and the op types)."""
    S = hm.scales
    steps = [("stem", "stem", {}), ("pool", "pool0", dict(x="stem"))]
    x, s_in = "pool0", S["stem"]
    for i, d in enumerate(hm.blocks):
        m = d["blk"]
        steps.append(("conv", f"r{i}_c1", dict(layer=m.conv1, x=x, s_in=s_in, s_out=S[f"b{i}.c1"])))
        steps.append(("conv", f"r{i}_c2", dict(layer=m.conv2, x=f"r{i}_c1", s_in=S[f"b{i}.c1"],
                                               s_out=S[f"b{i}.c2"])))
        idt = x
        if m.down is not None:
            steps.append(("conv", f"r{i}_down", dict(layer=m.down, x=x, s_in=s_in, s_out=S[f"b{i}.down"])))
            idt = f"r{i}_down"
        steps.append(("conv", f"r{i}_out", dict(layer=m.conv3, x=f"r{i}_c2", s_in=S[f"b{i}.c2"],
                                                s_out=S[f"b{i}.out"], res=idt, s_res=d["s_res"], act="relu")))
        x, s_in = f"r{i}_out", S[f"b{i}.out"]
    for kind, name in (("aspp", "aspp_cat"), ("gap", "gap"), ("pooled", "pooled"), ("img_bias", "img_bias"),
                       ("proj", "aspp_proj"), ("logits", "logits"), ("labels", "labels")):
        steps.append((kind, name, dict(x=x)))
    return steps


STAGES: Dict[str, Callable[[str], bool]] = {
    "stem_pool": lambda n: n in ("stem", "pool0"),
    "blocks0_6": lambda n: n[0] == "r" and int(n[1:].split("_")[0]) <= 6,
    "blocks7_15": lambda n: n[0] == "r" and int(n[1:].split("_")[0]) >= 7,
    "aspp_head": lambda n: n in ("aspp_cat", "gap", "pooled", "img_bias", "aspp_proj", "logits", "labels"),
}


def step_reference(hm, bufs, frames, lut_x, lut_y, kind: str, spec: dict, vname: str, rd,
                   interior: bool = True) -> torch.Tensor:
    """The exact expected output of one plan step, computed on device ``rd`` from the plan's
    own input buffers: int32 NCHW codes for the int8 steps, float64 for gap / pooled /
    img_bias / logits (NCHW), uint8 label maps for the labels."""
    from semantic_segmentation_server_amd.models.quant import _qw, int8_conv_codes
    from semantic_segmentation_server_amd.ops import reference_ops as R
    S = hm.scales
    a = hm.model.aspp

    def codes(name):  # a buffer's int8 NHWC codes as NCHW float on the reference device
        return _nchw(bufs[name]).to(rd).float()

    if kind == "stem":
        lut = lambda t: (t if torch.is_tensor(t) else torch.tensor(list(t))).to(rd)  # noqa: E731
        x = letterbox_pixels(frames.to(rd), lut(lut_x), lut(lut_y), stem_pixel_table())
        return stem_ref_codes(x, hm.model.backbone.stem, S["stem"], bf16_operands=vname != "fp32")
    if kind == "pool":
        return F.max_pool2d(codes(spec["x"]), 3, 2, 1).to(torch.int32)
    if kind == "conv":
        res = spec.get("res")
        return int8_conv_codes(spec["layer"], codes(spec["x"]), spec["s_in"], spec["s_out"],
                               None if res is None else codes(res), spec.get("s_res", 0.0),
                               act=spec.get("act"))
    if kind == "aspp":
        x = codes(spec["x"])
        branches = [int8_conv_codes(br, x, hm.s_feat, S["aspp.cat"], act="relu")
                    for br in [a.b0] + list(a.atrous)]
        if interior:
            for j, br in enumerate(branches):
                nz = (br != 0).double().mean().item()
                assert nz > 0.3, f"aspp branch {j}: only {nz:.3f} of the reference codes are non-zero"
        return torch.cat(branches, 1)
    if kind == "gap":
        return codes(spec["x"]).double().mean((2, 3)) * hm.s_feat
    if kind == "pooled":
        return torch.relu(bufs["gap"].to(rd).double() @ hm.pool_w.to(rd).double().t()
                          + hm.pool_b.to(rd).double())
    if kind == "img_bias":
        return bufs["pooled"].to(rd).double() @ hm.proj_pool_w.to(rd).double().t()
    if kind == "proj":
        wq, sw, b = _qw(a.project)
        v = exact_conv(codes("aspp_cat"), wq[:, :hm.cat_c], sw, b, S["aspp.cat"],
                       img_bias=bufs["img_bias"].to(rd), act="relu")
        return requant(v, S["aspp.proj"])
    if kind == "logits":
        wq, sw, b = _qw(hm.model.logits)
        return exact_conv(codes("aspp_proj"), wq, sw, b, S["aspp.proj"])
    if kind == "labels":
        lg = _nchw(bufs["logits"][..., :hm.num_classes]).to(rd).float()
        return R.upsample_argmax(lg, hm.H, hm.W)
    raise AssertionError(kind)


def check_plan(hm, ops, bufs, frames, lut_x, lut_y, *, run: bool = True, every_variant: bool = True,
               select: Optional[Callable[[str], bool]] = None, ref_device="cpu",
               interior: bool = True, chip_poison: Optional[Callable] = None) -> List[tuple]:
    """Walk a ``HipDeepLabInt8`` plan in order and check every step against exact arithmetic
    on the plan's OWN input buffers as they are at that moment (teacher forcing: nothing
    accumulates from step to step).

    ``run``: execute the ops -- a plain op once, a ``Choice`` through every entry of
    ``.variants`` (``every_variant``) or its pick alone; before each run the step's output
    buffer is filled with a sentinel (99 for int8, NaN for bf16 / fp32, 255 for the labels)
    so a pixel or channel the kernel skips is seen, and the last variant's output feeds the
    next step. ``run=False``: compare ``bufs`` as a finished run of the plan left them (a
    snapshot; the picks only). ``select(buffer name)``: the steps to check; the others are
    only executed. ``interior``: assert that the reference codes are not saturated (and the
    ASPP branches not dead), so a failure cannot hide behind a clamp.

    ``chip_poison``: a reproducibility walk instead, with no reference: every variant of every
    selected step runs three times from a sentinel-filled output, A, A' and, after
    ``chip_poison()`` (tests/chip_poison.py: every CU's LDS and every SIMD's registers NaN), P.
    A' != A is reported as "not reproducible", P != A with buffer, variant, the count of
    differing elements and the first index; bit-equal, no tolerance. What A is worth is the
    business of the walk above.

    Returns [(buffer, variant, share of codes off, max step)] for the int8 steps (the poisoned
    walk: one entry per (buffer, variant) that ran A / A' / P)."""
    from semantic_segmentation_server_amd.models.plan import Choice

    steps = plan_steps(hm)
    assert len(ops) == len(steps), (len(ops), len(steps))
    rd = torch.device(ref_device)
    report: List[tuple] = []
    failures: List[str] = []

    def check_interior(ref, what):
        if interior:
            sat = saturated_share(ref)
            assert sat < MAX_SATURATED, f"{what}: {sat:.3e} of the reference codes are saturated"

    def compare(kind, name, ref, what):
        out = bufs[name]
        if kind in ("stem", "pool", "conv", "aspp", "proj"):
            check_interior(ref, what)
            got = _nchw(out)
            if kind == "pool":
                assert torch.equal(got.to(torch.int32), ref), f"{what}: not bit-equal to F.max_pool2d"
                report.append((name, what.split("/")[-1], 0.0, 0))
            else:
                report.append((name, what.split("/")[-1]) + assert_codes_close(got, ref, what))
        elif kind == "gap":
            assert torch.allclose(out.double(), ref, rtol=1e-5, atol=0.0), what
        elif kind in ("pooled", "img_bias"):
            assert torch.allclose(out.double(), ref, rtol=1e-4, atol=1e-3), what
        elif kind == "logits":
            nc = hm.num_classes
            assert_bf16_close(_nchw(out[..., :nc]), ref, what)
            pad = out[..., nc:].float()
            if run:
                assert bool(torch.isnan(pad).all()), f"{what}: the padding channels {nc}.. were written"
            else:
                assert bool((pad == 0).all()), f"{what}: the padding channels {nc}.. were written"
        elif kind == "labels":
            agree = (out == ref).double().mean().item()
            assert agree > 0.9999, f"{what}: label agreement {agree:.6f}"

    for op, (kind, name, spec) in zip(ops, steps):
        is_choice = isinstance(op, Choice)
        assert is_choice == (kind in ("stem", "conv", "aspp", "proj", "logits")), (kind, name, type(op))
        if select is not None and not select(name):
            if run:
                op(frames, lut_x, lut_y)
            continue
        out = bufs[name]
        if not run:
            variants = [(op.variants[op.pick][0] if is_choice else "op", None)]
        elif is_choice:
            variants = op.variants if every_variant else [op.variants[op.pick]]
        else:
            variants = [("op", [op])]
        refs = {}
        if chip_poison is not None:
            assert run, "the reproducibility walk runs the ops"
            for vname, calls in variants:
                snaps = []
                for tag in ("A", "A'", "P"):
                    out.fill_(99 if out.dtype == torch.int8 else 255 if out.dtype == torch.uint8 else float("nan"))
                    if tag == "P":
                        chip_poison()
                    for c in calls:
                        c(frames, lut_x, lut_y)
                    if out.is_cuda:
                        torch.cuda.synchronize()
                    snaps.append(out if tag == "P" else out.clone())
                for tag, b in (("not reproducible: A' != A", snaps[1]), ("the poisoned run differs: P != A", snaps[2])):
                    d = CP.bit_diff(snaps[0], b)
                    if d is not None:
                        failures.append(f"{name}/{vname}: {tag} at {d[0]} of {out.numel()} elements, first at {d[1]}")
                report.append((name, vname, 0.0, 0))
            continue
        for vname, calls in variants:
            if calls is not None:
                out.fill_(99 if out.dtype == torch.int8 else 255 if out.dtype == torch.uint8 else float("nan"))
                for c in calls:
                    c(frames, lut_x, lut_y)
                if out.is_cuda:
                    torch.cuda.synchronize()
            form = vname != "fp32" if kind == "stem" else None  # the stem reference rounds as the kernel does
            if form not in refs:
                # compared where the buffer lives: a device-side compare costs two scalars per variant
                refs[form] = step_reference(hm, bufs, frames, lut_x, lut_y, kind, spec, vname, rd, interior).to(out.device)
            try:
                compare(kind, name, refs[form], f"{name}/{vname}")
            except AssertionError as e:  # report every failing (buffer, variant), not the first
                failures.append(str(e))
    assert not failures, f"{len(failures)} plan checks failed:\n" + "\n".join(failures)
    return report


def worst(report: List[tuple]) -> tuple:
    return max(report, key=lambda r: (r[3], r[2]))


def reference_ops(hm, ops, bufs, frames, lut_x, lut_y, only: Optional[Callable[[str], bool]] = None) -> list:
    """The plan's ops with every variant of every step replaced by a host function that writes
    the step's exact reference into its buffer (as ``fill_from_references`` does): a plan that
    ``check_plan(run=True)`` can walk on the CPU, into which a test injects a wrong op.
    ``only(buffer name)``: the steps that write; the others leave ``bufs`` as they are."""
    from semantic_segmentation_server_amd.models.plan import Choice
    rd = torch.device("cpu")
    out = []
    for op, (kind, name, spec) in zip(ops, plan_steps(hm)):
        def write(*args, kind=kind, name=name, spec=spec, vname="op"):
            if only is None or only(name):
                _write_reference(hm, bufs, frames, lut_x, lut_y, kind, name, spec, vname, rd)
        if isinstance(op, Choice):
            new = Choice(op.name, [(v, [lambda *a, v=v, w=write: w(vname=v)]) for v, _ in op.variants])
            new.pick = op.pick
            out.append(new)
        else:
            out.append(write)
    return out


def _write_reference(hm, bufs, frames, lut_x, lut_y, kind, name, spec, vname, rd):
    ref = step_reference(hm, bufs, frames, lut_x, lut_y, kind, spec, vname, rd, interior=False)
    out = bufs[name]
    if kind == "logits":
        out[..., :hm.num_classes] = ref.permute(0, 2, 3, 1).to(out.dtype)
    elif out.dim() == 4:
        out.copy_(ref.permute(0, 2, 3, 1).to(out.dtype))
    else:
        out.copy_(ref.to(out.dtype))


def fill_from_references(hm, ops, bufs, frames, lut_x, lut_y) -> None:
    """Write into ``bufs`` what a plan whose every kernel were exact would leave there (each
    step from the buffers before it): the walker's own CPU-tier test runs on this."""
    rd = torch.device("cpu")
    for op, (kind, name, spec) in zip(ops, plan_steps(hm)):
        vname = op.variants[op.pick][0] if hasattr(op, "variants") else "op"
        _write_reference(hm, bufs, frames, lut_x, lut_y, kind, name, spec, vname, rd)
