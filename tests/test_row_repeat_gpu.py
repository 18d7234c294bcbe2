"""The letterbox's constant rows computed once (csrc/hip/row_repeat.h): stem_band and
fused_ir_slice with the feature on are bit-identical to the feature off, at the kernel
level over zone / band layouts and at the plan level."""
import numpy as np
import pytest
import torch

from semantic_segmentation_server_amd.ops import row_repeat as RR

pytestmark = pytest.mark.gpu

DEV = "cuda"
B = 2


def _hip():
    from semantic_segmentation_server_amd.ops import hip_ops as K
    K._hip_mod()
    return K


def _nan(*shape):
    # NaN sentinel: a row left unwritten fails torch.equal (NaN != NaN) and the isfinite check
    return torch.full(shape, float("nan"), dtype=torch.bfloat16, device=DEV)


# ------------------------------------------------------------------------------ stem_band
STEM_H = 65  # model input 65 x 65, stem 33 x 33


def _stem_luts(case):
    """(Hc, Wc, lut_x, lut_y, zone of the 33 stem + block 0 rows)"""
    from semantic_segmentation_server_amd.ops import reference_ops as R_
    H = STEM_H
    cam = {"bottom": (80, 48), "square": (64, 64), "right": (48, 80), "allpad": (64, 64),
           "middle": (64, 64)}[case]
    lx, ly, *_ = R_.letterbox_luts(cam[0], cam[1], H, H)
    lx, ly = np.array(lx, dtype=np.int32), np.array(ly, dtype=np.int32)
    if case == "allpad":
        ly[:] = -1
    if case == "middle":  # a -1 run in the middle with valid rows after it: no zone
        ly[20:30] = -1
    zn = {"bottom": (21, 31), "square": None, "right": None, "allpad": (2, 31), "middle": None}[case]
    assert RR.zone(RR.pad_start(ly), H, 33, (2, 3, 3)) == zn
    if case == "bottom":
        assert RR.pad_start(ly) == 39
    return cam[1], cam[0], lx, ly


@pytest.fixture(scope="module")
def stem_packed():
    from semantic_segmentation_server_amd.models.layers import ConvBNAct, init_random
    from semantic_segmentation_server_amd.models.mobilenetv2 import InvertedResidual, IRSpec
    K = _hip()
    stem = ConvBNAct(3, 32, 3, 2, act="relu6")
    blk = InvertedResidual(IRSpec(32, 16, 1, 1, 1))
    init_random(stem, seed=5)
    init_random(blk, seed=6)
    g = torch.Generator().manual_seed(11)
    for m in list(stem.modules()) + list(blk.modules()):
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_mean.uniform_(-0.2, 0.2, generator=g)
            m.running_var.uniform_(0.5, 2.0, generator=g)
    stem.eval(); blk.eval()
    dwf, dbf = blk.dw.fold()
    pwf, pbf = blk.project.fold()
    return K.pack_stem_block0(stem, dwf[:, 0], dbf, pwf[:, :, 0, 0], pbf, DEV)


@pytest.mark.parametrize("case", ["bottom", "square", "right", "allpad", "middle"])
@pytest.mark.parametrize("nbx", [1, 2])
@pytest.mark.parametrize("R", [2, 5, 11, 33])
def test_stem_band_row_repeat(stem_packed, case, R, nbx):
    """R = 2 / 5 / 11 / 33 at the 80x48 camera's zone 21..30: a band start inside the zone,
    the zone start inside a band, a band across the zone's end, the whole map in one band."""
    K = _hip()
    Hc, Wc, lx, ly = _stem_luts(case)
    g = torch.Generator().manual_seed(4)
    fd = torch.randint(0, 256, (B, Hc, Wc, 3), generator=g, dtype=torch.uint8).to(DEV)
    lxd, lyd = torch.from_numpy(lx).to(DEV), torch.from_numpy(ly).to(DEV)
    for oneb in (True, False):
        off, on = _nan(B, 33, 33, 16), _nan(B, 33, 33, 16)
        K.stem_band(fd, lxd, lyd, stem_packed, off, H=STEM_H, W=STEM_H, R=R, nbx=nbx, one_barrier=oneb)
        K.stem_band(fd, lxd, lyd, stem_packed, on, H=STEM_H, W=STEM_H, R=R, nbx=nbx, one_barrier=oneb,
                    row_repeat=True)
        torch.cuda.synchronize()
        assert torch.isfinite(off).all() and torch.isfinite(on).all(), oneb
        assert torch.equal(on, off), (oneb, (on.float() - off.float()).abs().amax(dim=(0, 2, 3)).tolist())


# ------------------------------------------------------------------------- fused_ir_slice
@pytest.fixture(scope="module")
def slice_blocks():
    from test_fused_band_cpu import band_block, pack_band  # tests/ is on sys.path
    out = {}
    for form, (cin, cout, stride) in {"block2": (24, 24, 1), "block1": (16, 24, 2)}.items():
        blk, spec = band_block(cin, cout, stride, seed=cin * 5 + cout + stride)
        out[form] = (spec, pack_band(blk, spec, device=DEV))
    return out


@pytest.mark.parametrize("form", ["block2", "block1"])
@pytest.mark.parametrize("p0", [0, 12, 20, 31, 33])
@pytest.mark.parametrize("R", [2, 3, 7, 17, 33])
def test_fused_ir_slice_row_repeat(slice_blocks, form, p0, R):
    """The input taken as the model input (H = IH, rf = (stride, 1, 1)): rows >= p0 are one
    random row repeated, rows < p0 random."""
    from semantic_segmentation_server_amd.ops import fused_band as FB
    spec, packed = slice_blocks[form]
    IH = IW = 33
    stride = spec.stride
    OH, OW = (IH - 1) // stride + 1, (IW - 1) // stride + 1
    g = torch.Generator().manual_seed(37 + p0)
    x = torch.randn(B, IH, IW, spec.cin, generator=g).to(torch.bfloat16)
    if p0 < IH:
        x[:, p0:] = torch.randn(B, 1, IW, spec.cin, generator=g).to(torch.bfloat16)
    xd = x.contiguous().to(DEV)
    ly = torch.tensor([y if y < p0 else -1 for y in range(IH)], dtype=torch.int32, device=DEV)
    rf = (stride, 1, 1)
    widths = FB.slice_widths(spec.cin, spec.hidden, spec.cout, stride, 1)
    assert len(widths) == 2
    for nw in widths:
        for oneb in (False, True):
            off, on = _nan(B, OH, OW, spec.cout), _nan(B, OH, OW, spec.cout)
            kw = dict(B=B, IH=IH, IW=IW, stride=stride, residual=spec.residual, R=R, nw=nw, one_barrier=oneb)
            FB.fused_ir_slice(xd, packed, off, **kw)
            FB.fused_ir_slice(xd, packed, on, lut_y=ly, H=IH, rf=rf, **kw)
            torch.cuda.synchronize()
            assert torch.isfinite(off).all() and torch.isfinite(on).all(), (nw, oneb)
            assert torch.equal(on, off), (nw, oneb, (on.float() - off.float()).abs().amax(dim=(0, 2, 3)).tolist())


def test_slice_zones_of_the_cases():
    """The p0 values above give a whole-map zone, zones cut by the bands, and none."""
    assert RR.zone(0, 33, 33, (1, 1, 1)) == (1, 32)
    assert RR.zone(20, 33, 33, (1, 1, 1)) == (21, 32)
    assert RR.zone(31, 33, 33, (1, 1, 1)) is None
    assert RR.zone(33, 33, 33, (1, 1, 1)) is None
    assert RR.zone(12, 33, 17, (2, 1, 1)) == (7, 16)
    assert RR.zone(31, 33, 17, (2, 1, 1)) is None


# ----------------------------------------------------------------------------- plan level
def _pick_tallest(ops, Choice):
    """The row-streaming variant with the most rows per band in the stem and blocks 1-6;
    pick 0 elsewhere."""
    import re
    picks = {}
    for op in ops:
        if isinstance(op, Choice) and op.name in ("stem+block0",) + tuple(f"block{i}" for i in range(1, 7)):
            rows = [(int(m.group(1)), i) for i, (n, _) in enumerate(op.variants)
                    for m in [re.match(r"(?:stem_band|slice)(\d+)[xw]\d+o?$", n)] if m]
            assert rows, op.name
            op.pick = max(rows)[1]
            picks[op.name] = op.variants[op.pick][0]
    return picks


@pytest.mark.parametrize("cam", [(160, 120), (160, 90)])
def test_plan_row_repeat_switch(monkeypatch, cam):
    """MobileNetV2 at 129^2, B = 2, 160x120 camera (and 16:9, where blocks 3 and 4 have a zone too):
    logits and labels with SSA_ROW_REPEAT=0, with the default and with ``all`` (the repeat
    in the stem and in every slice block, with the plan's real cumulative receptive fields:
    stem -> block 1 -> block 2 (residual) -> block 3 -> block 6) are equal bit for bit."""
    from semantic_segmentation_server_amd import config as C
    from semantic_segmentation_server_amd.models.deeplab import build_model
    from semantic_segmentation_server_amd.models.hip_model import HipDeepLab
    from semantic_segmentation_server_amd.models.plan import Choice, HipPlanModel
    from semantic_segmentation_server_amd.ops import fused_band as FB
    from semantic_segmentation_server_amd.ops import reference_ops as R_
    # the same fixed picks in every plan (variants differ in rounding: no timing here)
    monkeypatch.setattr(HipPlanModel, "_autotune", lambda self, *a: setattr(self, "choices", {}))
    calls = []
    real_slice = FB.fused_ir_slice

    def spy(x, packed, out, **kw):
        calls.append((kw["IH"], kw["stride"], kw["R"], kw.get("lut_y") is not None, kw.get("rf")))
        return real_slice(x, packed, out, **kw)
    monkeypatch.setattr(FB, "fused_ir_slice", spy)
    S, (Wc, Hc) = 129, cam
    model = build_model("mnv2", 21, calibrate_hw=129)
    lx, ly, *_ = R_.letterbox_luts(Wc, Hc, S, S)
    p0 = RR.pad_start(ly)
    lxd = torch.tensor(np.array(lx), dtype=torch.int32, device=DEV)
    lyd = torch.tensor(np.array(ly), dtype=torch.int32, device=DEV)
    rng = np.random.default_rng(9)
    fd = torch.from_numpy(rng.integers(0, 256, (B, Hc, Wc, 3), dtype=np.uint8)).to(DEV)
    got, on = {}, {}
    for flag in ("0", None, "all"):
        if flag is None:
            monkeypatch.delenv("SSA_ROW_REPEAT", raising=False)
        else:
            monkeypatch.setenv("SSA_ROW_REPEAT", flag)
        hm = HipDeepLab(model, torch.device(DEV), C.Config(backend="hip", batch=B, input_size=S, graph=False))
        ops, _ = hm._plan(B, Hc, Wc)
        picks = _pick_tallest(ops, Choice)
        assert len(picks) == 7, picks
        del calls[:]
        logits = hm.logits(fd, lxd, lyd).clone()
        slices = list(calls)
        labels = hm.segment(fd, lxd, lyd).clone()
        torch.cuda.synchronize()
        assert [c[0] for c in slices] == [65, 33, 33, 17, 17, 17], slices  # blocks 1-6
        on[flag] = [c[3] for c in slices]
        got[flag] = (logits, labels)
        if flag == "all":
            # the case is not hollow: the receptive fields are the plan's own and the zones exist
            assert hm._block_rf(0) == (2, 3, 3) and RR.zone(p0, S, 65, (2, 3, 3)) is not None
            wide = cam == (160, 90)
            want_zone = [True, True, wide, wide, False, False]
            for (IH, stride, R, has_lut, rf), i, wz in zip(slices, range(1, 7), want_zone):
                assert has_lut and rf == hm._block_rf(i), (i, rf)
                OH = (IH - 1) // stride + 1
                assert (RR.zone(p0, S, OH, rf) is not None) == wz, (i, rf, RR.zone(p0, S, OH, rf))
    assert on["0"] == [False] * 6 and on["all"] == [True] * 6
    # default: the stride-2 blocks whose bands get shorter (none with this batch's 2-row bands)
    assert on[None] == [st == 2 and RR.pays(p0, S, (IH - 1) // st + 1, R, rf) for IH, st, R, _, rf in slices], on
    assert torch.isfinite(got["all"][0].float()).all()
    for flag in (None, "all"):
        assert torch.equal(got[flag][0], got["0"][0]), flag
        assert torch.equal(got[flag][1], got["0"][1]), flag
