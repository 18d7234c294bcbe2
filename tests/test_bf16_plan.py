"""Teacher-forced sweep of the bf16 plans (``HipDeepLab``), step by step, every kernel variant.

Every step of a plan -- stem + block 0 in all its fused forms, every MobileNetV2 block through
EVERY variant of its ``Choice`` (slice, band, stream / lattice / split-hidden, tile, row,
unfused with its nested expansion choice, dwp, dwproj), the ResNet stem forms, max pool and
convs, the ASPP branches (grouped, split-K with and without in-launch combine, with the pooling
branch as work items, separate with the nested per-branch choices), the pooling bias, the fused
head or projection + logits, and upsample + argmax -- is run on the GPU on the plan's own
buffers and compared, element by element, with a float64 reference of that step computed from
the step's input as the device left it (tests/plan_bound.py, tests/bound_cases.py). The bound
of each element is derived from the arithmetic, not tuned; a failure names buffer/variant and
the worst index. The plans are built without autotuning, so what is checked does not depend on
timing. Before each variant its output buffers are NaN; after it the ticket counters must be
zero again and the 0x5A guard bands of every plan buffer intact (``SSA_GUARD_BYTES``).

Shapes: ``mnv2-129`` (B = 3, 160 x 120: maps 65 / 33 / 17 / 9, partial tiles that straddle
images, split-K 2 / 3, landscape letterbox rows), ``mnv2-513`` (B = 2, 640 x 480: the 33-wide
maps of every stream, lattice and split-hidden variant, split-K 2 / 4 / 6, every ``+pool`` and
``head_g*`` form), ``mobile-129`` (the split head), ``resnet50-129`` (stem choice, max pool,
every conv_gemm step), ``mnv2-129-rr`` (``SSA_ROW_REPEAT=all``, against the references of
``mnv2-129``: the repeat must be invisible) and the committed picks of the tune file for the
headline B = 32 plan (16 copies each of two frames, references per distinct image) and the
B = 1 latency plan.

Measured on an MI355X (max |got - v| / e per stage; 1.000 is a rounding flip of exactly one ulp
at an element whose bound admits it, the largest any stage may show; "flips": the largest share
of a buffer's elements at which the bound admits a flip at all). Every id of every shape
passes: no bound is exceeded anywhere, the committed B = 32 and B = 1 picks included.
  mnv2-129 / mnv2-129-rr (identical figures; in the rr ids the row repeat was on in 12 of 12
    ``stem_band`` launches of the stem stage and in every slice launch, 9 per block stage, in
    the plain ids in none: the test spies on the launches and asserts it): stem + block 0
    1.000, flips 0.36; blocks 1-6 1.000, flips 0.43-0.66; blocks 7-16 1.000, flips 0.43-0.90 (76-84
    (buffer, variant) checks per block); ASPP 1.000 over 439 checks; head 0.000 (no element
    differs from v); labels: 2 winning classes on the plan's logits (margin scale 2.2,
    undecided 1.8e-4), 21 on the noise / smooth fields (undecided <= 5.4e-4), no decided pixel
    wrong in any variant.
  mnv2-513: stem + block 0 1.000, flips 0.38; blocks 1-6 1.000, flips 0.43-0.68; blocks 7-16
    1.000 over 131-179 checks per block (every stream / lattice / h{hs}[c] variant), flips
    0.86-1.00 (the fp16 depthwise chain's flips reach nearly every output of the wide blocks);
    ASPP 1.000 over 569 checks; head 1.000; labels 4 classes on the plan's logits (scale 3.0).
  mobile-129: as mnv2-129 in the backbone; ASPP 0.091, projection + logits 0.000.
  resnet50-129: stem 1.000 (fp32 and both MFMA forms), convs 1.000 (flips up to 0.86 in the
    last blocks), ASPP 0.143, head 0.000; labels: 1 class on the plan's logits (scale 118).
  picks-B32 / picks-B1: every stage 1.000 except block 16 (0.500); flips as mnv2-513.
Wall time per id after 0.3-0.5 s of setup per shape: 0.03-1.0 s at 129; at 513 blocks 4-16,
ASPP, head and upsample 0.3-1.8 s, and the 257^2 / 129^2 maps, whose CPU references cost
seconds, one id per reference family (whole they took 6.1 s (stem), 6.2 s (block 1), 9.0 s
(block 2) and 2.3 s (block 3)): stem 3.1 s (stem_block0) and 1.7 s (separate), block 1
1.1-1.4 s per family, block 2 3.2 s (band), 3.1 s (tile), 0.9 s (row), 0.8 s (unfused),
block 3 0.4-0.5 s; picks-B32 3.5 s at worst (block 2), picks-B1 0.5 s.
The whole module: 53 s without the poisoned ids below, which add 15 s.

``test_bf16_plan_poisoned`` (tests/chip_poison.py; the walk mode is ``chip_poison`` of
tests/plan_bound.py): the sweep shapes again, every leaf call of every variant at any depth three
times on the buffers it writes -- A, A' and P, the launch of P preceded by a fill of every CU's
LDS and every SIMD's registers with NaN -- with bit-equal outputs, fp32 partials and tickets
required, the upsample variants' label maps on the plan's logits and on the noise and smooth
fields included. No variant is left out and none is excused: measured on an MI355X, A = A' = P in
every one of the
  mnv2-129      649 leaf calls (20 ids, 0.07-0.16 s each; the first 0.65 s with the plan's build),
  mnv2-129-rr   102 leaf calls (7 ids: the launches that take the row repeat; 0.03-0.25 s),
  mnv2-513     1349 leaf calls (20 ids; stem and blocks 1-6 0.11-0.51 s, blocks 7-16 and ASPP,
                the stream / lattice / split-hidden variants, 0.52-0.79 s, head and upsample
                under 0.1 s: no id needs a split per family),
  mobile-129    643 leaf calls (20 ids, 0.08-0.19 s),
  resnet50-129  118 leaf calls (6 ids, 0.05-0.49 s),
the tickets zero again and the guard bands intact after every P. No variant's summation order
depends on arrival order (the in-launch combines sum their slabs in a fixed order): A' = A
everywhere, so no id falls back on the float64 bound. The LDS words these kernels read as an
index or address, and where each is written before it is read, are listed in
tests/test_chip_poison_gpu.py.
"""
import json

import numpy as np
import pytest
import torch

import plan_bound as PB

pytestmark = pytest.mark.gpu

DEV = "cuda"

# id -> (arch, aspp, input side, batch, camera width, camera height, SSA_ROW_REPEAT, tune-file key)
SHAPES = {
    "mnv2-129": ("mnv2", "full", 129, 3, 160, 120, None, None),
    "mnv2-129-rr": ("mnv2", "full", 129, 3, 160, 120, "all", None),
    "mnv2-513": ("mnv2", "full", 513, 2, 640, 480, None, None),
    "mobile-129": ("mnv2", "mobile", 129, 2, 160, 120, None, None),
    "resnet50-129": ("resnet50", "full", 129, 2, 160, 120, None, None),
    "picks-B32": ("mnv2", "full", 513, 32, 640, 480, None, "mnv2:B=32:cam=640x480:in=513"),
    "picks-B1": ("mnv2", "full", 513, 1, 640, 480, None, "mnv2:B=1:cam=640x480:in=513"),
}
_ASPP = ("aspp.branches", "aspp.b0", "aspp_cat", "img_bias", "gap", "pooled")
STAGES = {
    "stem": lambda n: n in ("stem+block0", "stem", "pool0"),
    **{f"block{i}": (lambda n, i=i: n == f"block{i}") for i in range(1, 17)},
    "blocks0_6": lambda n: n[0] == "r" and int(n[1:].split("_")[0]) <= 6,
    "blocks7_15": lambda n: n[0] == "r" and int(n[1:].split("_")[0]) >= 7,
    "aspp": lambda n: n in _ASPP or n.startswith("aspp.rate"),
    "head": lambda n: n in ("aspp.head", "aspp.proj", "logits"),
    "upsample": lambda n: n == "upsample",
}
_MNV2 = ["stem"] + [f"block{i}" for i in range(1, 17)] + ["aspp", "head", "upsample"]
_RESNET = ["stem", "blocks0_6", "blocks7_15", "aspp", "head", "upsample"]
_SLICED = ["stem"] + [f"block{i}" for i in range(1, 7)]  # the launches that take the row repeat
# mnv2-513: the float64 references of the 257^2 and 129^2 maps take seconds each on the CPU, so
# the stages of those maps are one id per reference family ("stage:family")
_SPLIT = {"stem": ("stem_block0", "separate"), "block1": ("band", "row", "tile", "unfused"),
          "block2": ("band", "row", "tile", "unfused"), "block3": ("band", "row", "tile", "unfused")}
_MNV2_513 = [f"{st}:{fam}" if st in _SPLIT else st for st in _MNV2 for fam in _SPLIT.get(st, (None,))]
PAIRS = [(s, st) for s in SHAPES for st in (
    _RESNET if s.startswith("resnet") else _SLICED if s.endswith("-rr") else _MNV2_513 if s == "mnv2-513" else _MNV2)]

_MODELS, _CACHES = {}, {}


def _env(mp, rr):
    """The plan's environment, held while the plan is built AND while its ops run: the stem band
    launches read ``SSA_ROW_REPEAT`` when they are called, the slice launches when they are built."""
    mp.setenv("SSA_GUARD_BYTES", "4096")
    for name in ("SSA_POOL_FORK", "SSA_POOL_FUSED", "SSA_FUSED_IR", "SSA_ROW_REPEAT"):
        mp.delenv(name, raising=False)
    if rr:
        mp.setenv("SSA_ROW_REPEAT", rr)


def _build(shape):
    from semantic_segmentation_server_amd import config as C
    from semantic_segmentation_server_amd.models.deeplab import build_model
    from semantic_segmentation_server_amd.models.hip_model import HipDeepLab
    from semantic_segmentation_server_amd.models.plan import TUNE_FILE_DEFAULT, all_choices
    from semantic_segmentation_server_amd.ops import reference_ops as R
    from semantic_segmentation_server_amd.runtime.sources import SyntheticSource
    arch, aspp, S, B, cw, ch, rr, key = SHAPES[shape]
    if (arch, aspp) not in _MODELS:
        _MODELS[arch, aspp] = build_model(arch, 21 if arch == "mnv2" else 19, aspp=aspp, calibrate_hw=65)
    model = _MODELS[arch, aspp]
    lx, ly, *_ = R.letterbox_luts(cw, ch, S, S)
    distinct = 2 if key else B
    f, _, _ = SyntheticSource(cw, ch, pool=distinct, seed=13).read_batch(distinct)
    frames = torch.from_numpy(np.array(f))
    frames = frames[torch.arange(B) % distinct].contiguous()  # picks-B32: 16 copies each of two frames
    cfg = C.Config(arch=arch, aspp=aspp, dtype="bf16", input_size=S, batch=B, backend="hip", graph=False,
                   num_classes=model.num_classes)
    with pytest.MonkeyPatch.context() as mp:  # no autotuning: deterministic and short
        mp.setattr(HipDeepLab, "_autotune", lambda self, *a: setattr(self, "choices", {}))
        _env(mp, rr)
        hm = HipDeepLab(model, torch.device(DEV), cfg)
        ops, bufs = hm._plan(B, ch, cw)
    assert {g[0] for g in hm._guards} >= {"logits", "labels", "aspp_cat"}, "the plan buffers have no guard bands"
    if key:  # the kernels the benchmark and the latency plan run
        with open(TUNE_FILE_DEFAULT) as fh:
            saved = json.load(fh)[key]
        every = all_choices(ops)
        for c in every:
            hit = [i for i, (n, _) in enumerate(c.variants) if n == saved.get(c.name)]
            assert hit, f"{key}: the saved pick {c.name}={saved.get(c.name)!r} is no variant of the plan"
            c.pick = hit[0]
        assert {c.name for c in every} == set(saved), sorted(set(saved) ^ {c.name for c in every})
    args = (frames.to(DEV).contiguous(), torch.tensor(lx.tolist(), dtype=torch.int32, device=DEV),
            torch.tensor(ly.tolist(), dtype=torch.int32, device=DEV))
    with pytest.MonkeyPatch.context() as mp:
        _env(mp, rr)
        for op in ops:  # one run of the picks: every stage starts from populated buffers
            op(*args)
        torch.cuda.synchronize()
    # the row-repeat plan is checked against the references of the plain plan of the same shape
    cache = _CACHES.setdefault((arch, aspp, S, B, cw, ch, key), {})
    return shape, hm, ops, bufs, args, key is None, cache


@pytest.fixture(scope="module")
def plans():
    """The plans by shape id, each built on first use and kept for the module."""
    built = {}
    yield lambda shape: built[shape] if shape in built else built.setdefault(shape, _build(shape))
    built.clear()
    _CACHES.clear()


@pytest.mark.parametrize("shape,stage", PAIRS, ids=[f"{s}-{st}" for s, st in PAIRS])
def test_bf16_plan(plans, shape, stage):
    """One stage of one plan (the other steps are only executed): every variant of every
    ``Choice`` of the sweep shapes, the committed picks of the tune-file plans."""
    from semantic_segmentation_server_amd.models.plan import Choice
    from semantic_segmentation_server_amd.ops import fused_band as FB
    from semantic_segmentation_server_amd.ops import hip_ops as K
    shape, hm, ops, bufs, (frames, lx, ly), every, cache = plans(shape)
    rr = SHAPES[shape][6]
    stage, _, fam = stage.partition(":")
    if fam:  # a stage split per family: its ids together cover every family the steps hold
        have = {PB.family(op.name, n) for op in ops if isinstance(op, Choice) and STAGES[stage](op.name)
                for n, _ in op.variants}
        assert have == set(_SPLIT[stage]), f"{shape} {stage}: families {sorted(have)}, ids for {_SPLIT[stage]}"
    repeat = {"stem_band": [], "fused_ir_slice": []}  # whether each row-streaming launch got the row repeat
    band, slice_ = K.stem_band, FB.fused_ir_slice
    with pytest.MonkeyPatch.context() as mp:
        _env(mp, rr)
        mp.setattr(K, "stem_band", lambda *a, **kw: (repeat["stem_band"].append(bool(kw["row_repeat"])), band(*a, **kw))[1])
        mp.setattr(FB, "fused_ir_slice", lambda *a, **kw: (repeat["fused_ir_slice"].append(kw.get("lut_y") is not None),
                                                          slice_(*a, **kw))[1])
        try:
            rep = PB.check_plan(hm, ops, bufs, frames, lx, ly, run=True, every_variant=every, select=STAGES[stage],
                                cache=cache, families={fam} if fam else None)
        except AssertionError:
            raise
        except RuntimeError as err:  # a device fault: nothing more is launched on this GPU
            pytest.exit(f"{shape} {stage}: {err}", returncode=3)
    assert rep, (shape, stage)
    if rr == "all":  # the repeat was really on, in every launch of the stage's own sweep
        kind = "stem_band" if stage == "stem" else "fused_ir_slice"
        assert len(repeat[kind]) >= 4 and all(repeat["stem_band"]) and all(repeat["fused_ir_slice"]), repeat
    w = PB.worst(rep)
    print(f"bf16 plan {shape} {stage} {fam}: {len(rep)} (buffer, variant) checks, worst ratio {w[2]:.3f} at "
          f"{w[0]}/{w[1]}, largest flip share {max(r[3] for r in rep):.3e}; row repeat on in "
          f"{sum(repeat['stem_band'])} / {len(repeat['stem_band'])} stem_band and "
          f"{sum(repeat['fused_ir_slice'])} / {len(repeat['fused_ir_slice'])} slice launches")


# ---------------------------------------------------------------- on poisoned LDS and registers
# The sweep shapes (the picks-* plans run the same kernels); the stages whole: no reference is
# computed, so no id needs a split per family.
POISON_SHAPES = ("mnv2-129", "mnv2-129-rr", "mnv2-513", "mobile-129", "resnet50-129")
POISON_PAIRS = [(s, st) for s in POISON_SHAPES for st in (
    _RESNET if s.startswith("resnet") else _SLICED if s.endswith("-rr") else _MNV2)]


@pytest.mark.parametrize("shape,stage", POISON_PAIRS, ids=[f"{s}-{st}" for s, st in POISON_PAIRS])
def test_bf16_plan_poisoned(plans, shape, stage):
    """One stage of one plan: every leaf call of every variant at any depth three times on the
    buffers it writes -- A, A' and, with every CU's LDS and every SIMD's registers NaN-filled just
    before the launch, P (tests/chip_poison.py): bit-equal outputs, partials and tickets, the
    tickets zero again and the guard bands intact after P. The A outputs are those the ids of
    ``test_bf16_plan`` hold to their float64 bounds."""
    import chip_poison as CP
    CP.require()
    shape, hm, ops, bufs, (frames, lx, ly), every, cache = plans(shape)
    assert every
    from semantic_segmentation_server_amd.ops import fused_band as FB
    from semantic_segmentation_server_amd.ops import hip_ops as K
    rr = SHAPES[shape][6]
    repeat = []  # whether each row-streaming launch got the row repeat
    band, slice_ = K.stem_band, FB.fused_ir_slice
    with pytest.MonkeyPatch.context() as mp:
        _env(mp, rr)
        mp.setattr(K, "stem_band", lambda *a, **kw: (repeat.append(bool(kw["row_repeat"])), band(*a, **kw))[1])
        mp.setattr(FB, "fused_ir_slice", lambda *a, **kw: (repeat.append(kw.get("lut_y") is not None), slice_(*a, **kw))[1])
        wk = PB.Walker(hm, ops, bufs, frames, lx, ly, run=True, every_variant=True, select=STAGES[stage],
                       chip_poison=CP.poison)
        try:
            rep = wk.walk()
        except AssertionError:
            raise
        except RuntimeError as err:  # a device fault: nothing more is launched on this GPU
            pytest.exit(f"{shape} {stage} poisoned: {err}", returncode=3)
    assert rep and wk.leaves == len(rep), (shape, stage, wk.leaves, len(rep))
    if rr == "all":  # the repeat was really on, in every row-streaming launch of the stage, P included
        assert len(repeat) >= 12 and all(repeat), repeat
    print(f"bf16 plan {shape} {stage} poisoned: {wk.leaves} leaf calls, A = A' = P in all of them; row repeat on in "
          f"{sum(repeat)} / {len(repeat)} row-streaming launches")
