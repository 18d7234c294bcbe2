"""Plan machinery of the HIP models (``hip_model.HipDeepLab``, ``hip_int8.HipDeepLabInt8``).

A plan is a fixed list of kernel launches over static buffers, built once per (batch,
camera); a step with alternative implementations is a ``Choice``. The names of the choices
and of their variants are a contract with the tune file: a saved name that no longer exists
is re-timed at start-up, which changes the kernels that run (tests/test_plan_cpu.py).
"""
from __future__ import annotations

import json
import math
import os
import sys
from typing import Callable, Dict, List, Optional, Tuple

import torch

# committed plan picks for MI355X (plan shapes of the headline and the BASELINE configs)
TUNE_FILE_DEFAULT = os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(
    os.path.abspath(__file__)))), "assets", "tune_mi355x.json")


class Choice:
    """A plan step with alternative implementations; ``autotune`` keeps the
    fastest on the actual shapes (timed with HIP events at plan build)."""

    def __init__(self, name: str, variants: List[Tuple[str, List[Callable]]]):
        self.name = name
        self.variants = variants
        self.pick = 0

    def __call__(self, *args):
        for op in self.variants[self.pick][1]:
            op(*args)

    def autotune(self, args, reps: int = 5) -> None:
        mode = os.environ.get("SSA_FUSED_IR", "auto")
        if mode in ("0", "1"):
            want = "unfused" if mode == "0" else "fused"
            self.pick = next((i for i, (n, _) in enumerate(self.variants) if n == want), 0)
            for _, ops in self.variants:
                for op in ops:
                    if isinstance(op, Choice):
                        op.autotune(args, reps)
            return
        for _, ops in self.variants:  # nested choices first (e.g. block 0 inside stem+block0)
            for op in ops:
                if isinstance(op, Choice):
                    op.autotune(args, reps)
        if len(self.variants) < 2:
            return
        times = []
        graph = os.environ.get("SSA_TUNE_GRAPH", "1") == "1"
        for _, ops in self.variants:
            for _ in range(2):
                for op in ops:
                    op(*args)
            st, en = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            g = None
            if graph:
                # time the variant replayed from a hipGraph, as the engine runs it: timed from
                # Python, every kernel under ~16 us measured the host's launch path instead
                # (all batch-1 variants of blocks 7-10 read 16-17 us, r4 retune tables)
                torch.cuda.synchronize()
                g = torch.cuda.CUDAGraph()
                # thread-local capture: a plan built lazily while another thread (feeder,
                # result collector) uses the device must not invalidate their calls
                with torch.cuda.graph(g, capture_error_mode="thread_local"):
                    for _ in range(reps):
                        for op in ops:
                            op(*args)
                g.replay()
            st.record()
            if g is not None:
                g.replay()
            else:
                for _ in range(reps):
                    for op in ops:
                        op(*args)
            en.record()
            en.synchronize()
            times.append(st.elapsed_time(en) / reps)
            del g
        self.pick = min(range(len(times)), key=times.__getitem__)
        self.times = times


def all_choices(ops: List[Callable]) -> List[Choice]:
    """The top-level choices of a plan, then the choices nested in their variants."""
    top = [op for op in ops if isinstance(op, Choice)]
    return top + [o for c in top for _, vops in c.variants for o in vops if isinstance(o, Choice)]


def copy_picks(src: List[Callable], dst: List[Callable]) -> None:
    """Give every Choice of ``dst`` (a plan built by the same code) the pick of the
    Choice at the same position in ``src``, nested choices included."""
    for a, b in zip(src, dst):
        if isinstance(a, Choice) and isinstance(b, Choice):
            b.pick = a.pick
            for (_, va), (_, vb) in zip(a.variants, b.variants):
                copy_picks(va, vb)


class HipPlanModel:
    """Base of the HIP models: the plans per (batch, camera[, part]), their tuning, ``segment``.

    A subclass packs its weights, sets ``kind`` (the tune-file key prefix) and implements
    ``_build(B, Hc, Wc, buf, bufs) -> ops``. ``buf(name, *shape, dtype=buf_dtype)`` allocates
    a zeroed plan buffer into ``bufs``, "logits" and "labels" among them; the last op writes
    ``self._labels_out if self._labels_out is not None else labels``. With ``confidence`` the
    plan also has a "conf" buffer (uint8 [B, H, W] codes, ``reference_ops.upsample_confidence``)
    and its last op writes both planes (``_final_op``)."""

    kind = ""
    buf_dtype = torch.bfloat16

    def __init__(self, model, device: torch.device, input_size: int, confidence: bool = False):
        self.device = device
        self.confidence = bool(confidence)
        self._conf_out: Optional[torch.Tensor] = None  # segment(conf_out=): caller's conf plane
        self.model = model
        self.H = self.W = int(input_size)
        self.num_classes = model.num_classes
        self.ldk = (self.num_classes + 7) // 8 * 8
        # set by the DP pipeline at world > 1: rank 0's autotune picks -> every rank
        self.pick_sync: Optional[Callable[[Optional[dict]], dict]] = None
        self.choices: Dict[str, str] = {}  # step name -> picked variant of the last tuned plan
        self._plans: Dict[tuple, Tuple[List[Callable], Dict[str, torch.Tensor]]] = {}
        self._labels_out: Optional[torch.Tensor] = None  # segment(out=): caller's label maps
        self._guards: list = []  # SSA_GUARD_BYTES debug bands (name, raw, guard, nbytes)

    # ------------------------------------------------------------------ plan
    def _plan(self, B: int, Hc: int, Wc: int, part: int = 0):
        """Kernel list + static buffers for (B, camera). ``part`` > 0: an independent
        copy (own buffers) of the same plan, for concurrent sub-batches on separate
        streams; it takes part 0's autotune picks."""
        key = (B, Hc, Wc) if part == 0 else (B, Hc, Wc, part)
        if key in self._plans:
            return self._plans[key]
        bufs: Dict[str, torch.Tensor] = {}
        ops = self._build(B, Hc, Wc, self._allocator(bufs), bufs)
        self._plans[key] = (ops, bufs)
        if part == 0:
            self._autotune(ops, B, Hc, Wc)
        else:
            copy_picks(self._plan(B, Hc, Wc)[0], ops)
            # first launches (lazy kernel attributes) outside any capture
            self._launch(ops, self._tune_inputs(B, Hc, Wc))
            torch.cuda.synchronize(self.device)
        return self._plans[key]

    def _allocator(self, bufs: Dict[str, torch.Tensor]) -> Callable:
        dev = self.device
        guard = int(os.environ.get("SSA_GUARD_BYTES", "0"))  # debug: sentinel bands

        def buf(name, *shape, dtype=self.buf_dtype):
            # zeroed for tidiness only (and so that plan copies start identical): no picked
            # kernel reads plan bytes it did not write
            # (plan constants kept among the buffers are named const_*, pool_w*)
            # (scripts/debug_poison.py run B: NaN-filled buffers give bit-identical labels;
            # tests/test_hip_kernels.py::test_plan_is_a_function_of_the_frame, at 257^2 and
            # at the headline 513^2 / 640x480 shape with the B = 32 plan's kernels)
            if guard:  # debug (scripts/debug_guard.py): 0x5A bands before and after
                nb = math.prod(shape) * torch.tensor([], dtype=dtype).element_size()
                raw = torch.full((nb + 2 * guard,), 0x5A, dtype=torch.uint8, device=dev)
                raw[guard:guard + nb].zero_()
                t = raw[guard:guard + nb].view(dtype).view(*shape)
                self._guards.append((name, raw, guard, nb))
            else:
                t = torch.zeros(shape, dtype=dtype, device=dev)
            bufs[name] = t
            return t
        return buf

    def _final_op(self, buf, logits, B, h, w, variants):
        """The plan's last step: ``upsample_argmax`` as the "upsample" choice over ``variants``,
        or with ``confidence`` one plain op that writes the labels and the "conf" buffer."""
        from ..ops import hip_ops as K
        H, W = self.H, self.W
        labels = buf("labels", B, H, W, dtype=torch.uint8)
        if self.confidence:
            conf = buf("conf", B, H, W, dtype=torch.uint8)
            return [lambda *_: K.upsample_argmax_conf(
                logits, self._labels_out if self._labels_out is not None else labels,
                self._conf_out if self._conf_out is not None else conf, B=B, h=h, w=w,
                K=self.num_classes, ldk=self.ldk, H=H, W=W)]
        ups = [(name, [lambda *_, v=K.UPSAMPLE_VARIANTS[name]: K.upsample_argmax(
            logits, self._labels_out if self._labels_out is not None else labels, B=B, h=h, w=w,
            K=self.num_classes, ldk=self.ldk, H=H, W=W, variant=v)]) for name in variants]
        return [Choice("upsample", ups)] if len(ups) > 1 else ups[0][1]

    @staticmethod
    def _launch(ops: List[Callable], args) -> None:
        for op in ops:
            op(*args)

    def _tune_inputs(self, B: int, Hc: int, Wc: int):
        """Representative autotune inputs: letterboxed synthetic camera frames (the
        bench/serving source) and the real letterbox LUTs. All-zero frames would make
        the data-dependent kernels (upsample's convexity shortcut, the post stage)
        take their degenerate fast paths (VERDICT r1 Weak #9)."""
        import numpy as np
        from ..ops import reference_ops as R
        from ..runtime.sources import SyntheticSource
        src = SyntheticSource(Wc, Hc, stream=0, seed=1234, pool=min(B, 4))
        fr, _, _ = src.read_batch(B)
        frames = torch.from_numpy(np.ascontiguousarray(fr)).to(self.device)
        lx, ly, *_ = R.letterbox_luts(Wc, Hc, self.W, self.H)
        return (frames, torch.tensor(np.array(lx), dtype=torch.int32, device=self.device),
                torch.tensor(np.array(ly), dtype=torch.int32, device=self.device))

    # -------------------------------------------------------------- autotune
    def _autotune(self, ops, B, Hc, Wc) -> None:
        """Time every Choice on the real buffers and keep the fastest variant.

        Picks come, in order, from: ``SSA_TUNE_FILE=path.json`` (or, unset, the
        committed ``assets/tune_mi355x.json``), keyed by plan shape, so a deployment and
        the driver's short benchmark run reuse one fixed plan instead of re-timing at
        start-up (timings are noisy and variants differ in rounding; the int8 variants by
        up to one requantisation step); else from timing on representative inputs -- on
        rank 0 only when ``pick_sync`` is set (the DP pipeline broadcasts rank 0's picks,
        so every rank runs the same kernels and produces the same label maps). With
        SSA_TUNE_FILE set, newly timed picks are written back (rank 0, atomic replace)."""
        if torch.cuda.is_current_stream_capturing():
            return
        args = self._tune_inputs(B, Hc, Wc)
        self._launch(ops, args)  # populate every buffer once
        every = all_choices(ops)
        key = f"{self.kind}:B={B}:cam={Wc}x{Hc}:in={self.H}"
        env_path = os.environ.get("SSA_TUNE_FILE")
        path = env_path or TUNE_FILE_DEFAULT
        saved = self._saved_picks(path, key)
        rank0 = int(os.environ.get("RANK", "0")) == 0
        timed = self._apply_or_time(ops, every, saved, args, rank0)
        if timed and self.pick_sync is not None:
            # (with saved picks every rank reads the same file, so every rank re-timed the
            # same choices: the broadcast is collective) rank 0's timings decide
            picks = self.pick_sync({op.name: op.pick for op in every} if rank0 else None)
            for op in every:
                op.pick = picks.get(op.name, op.pick)
        torch.cuda.synchronize(self.device)
        self.choices = {op.name: op.variants[op.pick][0] for op in every}
        if env_path and timed and rank0:
            self._write_picks(env_path, key)
        if os.environ.get("SSA_LOG_AUTOTUNE", "0") == "1":
            self._log_picks(ops, B, path if saved else None)

    @staticmethod
    def _saved_picks(path: str, key: str) -> dict:
        if path and os.path.exists(path) and os.environ.get("SSA_RETUNE", "0") != "1":
            with open(path) as f:
                return json.load(f).get(key, {})
        return {}

    def _apply_or_time(self, ops, every, saved: dict, args, rank0: bool) -> bool:
        """Set the saved picks and time what they do not cover; True if anything was timed."""
        top = [op for op in ops if isinstance(op, Choice)]
        if not saved:  # cold: time every top-level choice (nested ones with their parent)
            if self.pick_sync is None or rank0:
                for op in top:
                    op.autotune(args)
            return True
        # SSA_RETUNE_ONLY=block7,block8,...: re-time just these choices (exact names) on top
        # of the saved picks (a new kernel variant for a few plan steps)
        only = {n for n in os.environ.get("SSA_RETUNE_ONLY", "").split(",") if n}
        retimed = False
        for op in every:
            hit = next((i for i, (n, _) in enumerate(op.variants) if n == saved.get(op.name)), None)
            tunable = op in top and len(op.variants) > 1
            if tunable and (op.name in only or hit is None):
                op.autotune(args)  # asked for, or a variant set the saved plan does not know
                retimed = True
            elif hit is not None:
                op.pick = hit
        return retimed

    def _write_picks(self, path: str, key: str) -> None:
        allp = {}
        if os.path.exists(path):
            with open(path) as f:
                allp = json.load(f)
        allp[key] = self.choices
        tmp = f"{path}.{os.getpid()}.tmp"
        with open(tmp, "w") as f:
            json.dump(allp, f, indent=1, sort_keys=True)
        os.replace(tmp, path)

    def _log_picks(self, ops, B: int, saved_path: Optional[str]) -> None:
        for op in ops:
            if isinstance(op, Choice) and hasattr(op, "times"):
                print(f"[autotune B={B}] {op.name}: " + ", ".join(
                    f"{n}={t * 1e3:.1f}us" for (n, _), t in zip(op.variants, op.times)) +
                    f" -> {op.variants[op.pick][0]}", file=sys.stderr)
        if saved_path:
            print(f"[autotune B={B}] picks from {saved_path}: {self.choices}", file=sys.stderr)

    # ------------------------------------------------------------------ run
    def segment(self, frames: torch.Tensor, lut_x: torch.Tensor, lut_y: torch.Tensor,
                out: Optional[torch.Tensor] = None, part: int = 0,
                conf_out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """frames: (B, Hc, Wc, 3) uint8 BGR on device -> (B, H, W) uint8 labels (static
        buffer, or ``out``). ``part``: which independent copy of the plan to run (the
        engine's concurrent half-batches use parts 0 and 1). A model built with ``confidence``
        also writes the confidence plane, into the plan's "conf" buffer or ``conf_out``."""
        B, Hc, Wc, _ = frames.shape
        if lut_x.numel() != self.W or lut_y.numel() != self.H:
            raise ValueError("letterbox LUTs do not match the model input size")
        ops, bufs = self._plan(B, Hc, Wc, part)
        if out is not None and (out.shape != bufs["labels"].shape or out.dtype != torch.uint8
                                or not out.is_contiguous() or out.device != bufs["labels"].device):
            raise ValueError("segment: out must match the (B, H, W) uint8 label buffer")
        if conf_out is not None:
            if not self.confidence:
                raise ValueError("segment: conf_out needs a model built with confidence")
            if (conf_out.shape != bufs["conf"].shape or conf_out.dtype != torch.uint8
                    or not conf_out.is_contiguous() or conf_out.device != bufs["conf"].device):
                raise ValueError("segment: conf_out must match the (B, H, W) uint8 conf buffer")
        frames = frames.contiguous()
        self._labels_out, self._conf_out = out, conf_out
        try:
            for op in ops:
                op(frames, lut_x, lut_y)
        finally:
            self._labels_out = self._conf_out = None
        return bufs["labels"] if out is None else out

    def logits(self, frames, lut_x, lut_y) -> torch.Tensor:
        """Run and return the NHWC logits buffer (tests)."""
        self.segment(frames, lut_x, lut_y)
        B, Hc, Wc, _ = frames.shape
        return self._plans[(B, Hc, Wc)][1]["logits"][..., : self.num_classes]

    def buffers(self, B: int, Hc: int, Wc: int) -> Dict[str, torch.Tensor]:
        return self._plan(B, Hc, Wc)[1]
