"""Teacher-forced sweep of the whole int8 DeepLabv3-ResNet50 plan, every kernel variant.

Every step of a ``HipDeepLabInt8`` plan -- the int8 stem in all its kernel forms, the int8
max pool, every conv ``Choice`` through EVERY ``conv_i8`` variant it offers, the ASPP
branches in their separate and grouped forms, the pooled branch as a per-image bias, the
projection, the bf16 logits and the label map -- is run on the GPU and compared with exact
arithmetic on the plan's own input buffers (tests/int8_ref.py: ``check_plan``). The plan
is built without autotuning, so which kernels are checked does not depend on timing.

Bounds: int8 codes at most one step off the exact reference on at most 1e-3 of a tensor's
codes (the pool bit-equal); gap rtol 1e-5, the matvecs rtol 1e-4 / atol 1e-3; bf16 logits
within 2^-8 relative + 1e-6 elementwise with the row padding untouched; labels > 0.9999.

The stem reference normalises pixels with ONE rounding, fp32(p * fp32(1 / 127.5) - 1):
``stem_conv``, ``stem_mfma`` (all tile forms) and ``stem_band`` all compile ``px * (1.f /
127.5f) - 1.f`` to a single v_fma_f32 (read from the gfx950 ISA of csrc/hip/model_ops.hip
and csrc/hip/stem_band.hip); ``reference_ops.preprocess`` rounds twice, which moves one of
the 256 values to another bf16 (tests/test_quant_cpu.py::test_stem_pixel_table_forms).
The MFMA forms are checked against both operands rounded to bf16, the per-lane form against
fp32 operands, both accumulated in float64.

Measured on an MI355X (share of codes one step off, never more than one step): at 129^2 the
worst (buffer, variant) is r11_c1 with every LDS-DMA and streaming variant at 4.8e-5
(register-fed v1: 8.0e-6 at worst), the stem 1.2e-6 (fp32) / 0 (MFMA forms), ASPP and
projection 0; at 321^2 r11_out at 1.1e-5, the stem 9.0e-7 / 6.0e-7, both ASPP forms 4.4e-6.
Each test id runs in 0.05-0.3 s after 0.5-0.8 s of setup per shape.

``test_int8_plan_poisoned`` (tests/chip_poison.py, ``check_plan(chip_poison=...)``): the 129 plan
again, every variant of every step three times from a sentinel-filled output -- A, A' and P, the
launches of P preceded by a fill of every CU's LDS and every SIMD's registers with NaN -- and
the outputs bit-equal. Measured on an MI355X: A = A' = P in all 692 (buffer, variant) calls (8
stem and pool, 299 + 357 convs through every ``conv_i8`` variant, the LDS-DMA ones included, 28
ASPP, pooling, projection, logits and labels); no variant is left out; 0.01-0.07 s per id.
"""
import numpy as np
import pytest
import torch

import int8_ref as I

pytestmark = pytest.mark.gpu

DEV = "cuda"

# (input side, batch, camera width, camera height): the smallest shapes at which the named
# logic is live.
#  129 / B = 3: maps 65 -> 33 -> 17 -> 9, M = 243 at 9 x 9: every tile height (96 / 128 /
#    160 / 256) is partial and straddles image boundaries (per-image bias index, m >= M).
#  321 / B = 2, portrait camera: maps 161 -> 81 -> 41 -> 21: at 21 x 21 the rates 6 / 12 / 18
#    all have live off-centre taps and several border classes; M = 13 122 at 81 x 81 reaches
#    the register-fed kernel's wide form and full tiles.
SHAPES = {"129": (129, 3, 160, 120), "321": (321, 2, 150, 200)}


@pytest.fixture(scope="module", params=list(SHAPES))
def plan(request):
    from semantic_segmentation_server_amd import config as C
    from semantic_segmentation_server_amd.models.deeplab import build_model
    from semantic_segmentation_server_amd.models.hip_int8 import HipDeepLabInt8
    from semantic_segmentation_server_amd.models.quant import calibrate
    from semantic_segmentation_server_amd.ops import reference_ops as R
    from semantic_segmentation_server_amd.runtime.sources import SyntheticSource
    S, B, cw, ch = SHAPES[request.param]
    model = build_model("resnet50", 19, calibrate_hw=65)
    lx, ly, *_ = R.letterbox_luts(cw, ch, S, S)
    f, _, _ = SyntheticSource(cw, ch, pool=B, seed=13).read_batch(B)
    frames = torch.from_numpy(np.array(f))
    scales = calibrate(model.float(), R.preprocess(frames, lx, ly))  # the evaluation frames: interior codes
    cfg = C.Config(arch="resnet50", dtype="int8", input_size=S, batch=B, backend="hip", graph=False,
                   num_classes=19)
    with pytest.MonkeyPatch.context() as mp:  # no autotuning: deterministic and short
        mp.setattr(HipDeepLabInt8, "_autotune", lambda self, *a: setattr(self, "choices", {}))
        hm = HipDeepLabInt8(model, torch.device(DEV), cfg, scales=scales)
        ops, bufs = hm._plan(B, ch, cw)
    args = (frames.to(DEV).contiguous(), torch.tensor(lx.tolist(), dtype=torch.int32, device=DEV),
            torch.tensor(ly.tolist(), dtype=torch.int32, device=DEV))
    for op in ops:  # one run of the default picks: every stage starts from populated buffers
        op(*args)
    torch.cuda.synchronize()
    return request.param, hm, ops, bufs, args


@pytest.mark.parametrize("stage", list(I.STAGES))
def test_int8_plan_every_variant(plan, stage):
    """One stage of the plan (the other steps are only executed), every variant of every
    ``Choice``; the assertion message names the buffer and the variant."""
    shape, hm, ops, bufs, (frames, lx, ly) = plan
    rep = I.check_plan(hm, ops, bufs, frames, lx, ly, run=True, every_variant=True,
                       select=I.STAGES[stage])
    assert rep, stage
    by_variant = {}
    for name, v, share, mx in rep:
        by_variant.setdefault(v, []).append((share, mx, name))
    print(f"int8 plan {shape} {stage}: {len(rep)} (buffer, variant) checks, worst {I.worst(rep)}; per variant "
          + ", ".join(f"{v} {max(r)[0]:.1e}" for v, r in sorted(by_variant.items())))


@pytest.mark.parametrize("plan", ["129"], indirect=True)
@pytest.mark.parametrize("stage", list(I.STAGES))
def test_int8_plan_poisoned(plan, stage):
    """One stage of the 129 plan (every tile height partial and straddling images): every variant
    of every step three times from a sentinel-filled output -- A, A' and, with every CU's LDS and
    every SIMD's registers NaN-filled just before the launches, P (tests/chip_poison.py): the
    codes bit-equal, no tolerance. The A outputs are those ``test_int8_plan_every_variant``
    holds to the exact codes."""
    import chip_poison as CP
    CP.require()
    shape, hm, ops, bufs, (frames, lx, ly) = plan
    try:
        rep = I.check_plan(hm, ops, bufs, frames, lx, ly, run=True, every_variant=True, select=I.STAGES[stage],
                           chip_poison=CP.poison)
    except AssertionError:
        raise
    except RuntimeError as err:  # a device fault: nothing more is launched on this GPU
        pytest.exit(f"int8 {shape} {stage} poisoned: {err}", returncode=3)
    assert rep, stage
    print(f"int8 plan {shape} {stage} poisoned: {len(rep)} (buffer, variant) calls, A = A' = P in all of them")


def test_conv_i8_refuses_what_it_cannot_do():
    """The wrappers refuse the shapes a variant cannot do instead of running them."""
    from semantic_segmentation_server_amd.ops import hip_ops as K
    x = torch.zeros(1, 4, 4, 64, dtype=torch.int8, device=DEV)
    w = torch.zeros(24, 64, dtype=torch.int8, device=DEV)
    sc, bi = torch.ones(24, device=DEV), torch.zeros(24, device=DEV)
    out = torch.zeros(1, 4, 4, 24, dtype=torch.int8, device=DEV)
    kw = dict(B=1, IH=4, IW=4, Cin=64, OH=4, OW=4, Cout=24, out_scale=0.1)
    for v in (5, 6, 10, 11):  # streaming forms need Cout % 16 == 0
        with pytest.raises(ValueError):
            K.conv_i8(x, w, sc, bi, out, variant=v, **kw)
    with pytest.raises(ValueError):  # a row permutation needs an LDS-DMA variant
        K.conv_i8(x, w, sc, bi, out, variant=1, perm=torch.zeros(128, dtype=torch.int32, device=DEV), **kw)
    with pytest.raises(ValueError):
        K.conv_i8(x, w, sc, bi, out, variant=2, **dict(kw, ldo=16))
    assert int(out.abs().max()) == 0
