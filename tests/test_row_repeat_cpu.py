"""ops/row_repeat.py (the host mirror of csrc/hip/row_repeat.h): the zone of output rows
that equal the row above them under a bottom letterbox, against brute force."""
import pytest
import torch
import torch.nn.functional as F

from semantic_segmentation_server_amd.ops import row_repeat as RR

STRIDES = (2, 1, 2, 1, 2)


def _p0s(H):
    return [0, 1, H // 3, H // 2 + 1, H - 9, H - 2, H - 1, H]


@pytest.mark.parametrize("H", [33, 65, 129])
def test_zone_rows_equal_brute_force(H):
    """A chain of 3x3 pad-1 convs with integer weights on an integer-valued letterboxed
    input, in float64 (exact): every row inside the predicted zone equals row z0, and the
    row above the zone does not (the zone starts as early as it can)."""
    g = torch.Generator().manual_seed(H)
    W, C = 11, 2
    ws = [torch.randint(-3, 4, (C, C, 3, 3), generator=g).double() for _ in STRIDES]
    bs = [torch.randint(-2, 3, (C,), generator=g).double() for _ in STRIDES]
    for p0 in _p0s(H):
        x = torch.randint(-5, 6, (1, C, H, W), generator=g).double()
        x[:, :, p0:] = -1.0
        lut = [y if y < p0 else -1 for y in range(H)]
        assert RR.pad_start(lut) == p0
        rf, zones = RR.RF_INPUT, 0
        for w, b, s in zip(ws, bs, STRIDES):
            x = F.conv2d(x, w, b, stride=s, padding=1)
            rf = RR.rf_conv3x3(rf, s)
            OH = x.shape[2]
            zn = RR.zone(p0, H, OH, rf)
            if zn is None:
                continue
            zones += 1
            z0, z1 = zn
            assert 0 <= z0 and z1 <= OH and z1 - z0 >= 2
            for o in range(z0 + 1, z1):
                assert torch.equal(x[0, :, o], x[0, :, z0]), (p0, rf, o)
            if z0 > 0 and p0 > 0:
                assert not torch.equal(x[0, :, z0 - 1], x[0, :, z0]), (p0, rf)
        assert zones > 0 or p0 >= H - 9


def test_pad_start_is_the_trailing_run():
    assert RR.pad_start([0, 1, -1, -1, 2, -1, -1]) == 5  # a -1 run in the middle: not pad
    assert RR.pad_start([-1, -1, -1]) == 0
    assert RR.pad_start([0, 1, 2]) == 3


def test_headline_zones():
    """513^2 model input, 640x480 camera (rows 384..512 pad): the identical rows of the stem
    + block 0 output and of blocks 1-6."""
    H, p0 = 513, 384
    rf = RR.rf_conv3x3(RR.rf_conv3x3(RR.RF_INPUT, 2))  # stem s2, block 0
    assert rf == (2, 3, 3)
    oh = 257
    assert RR.zone(p0, H, oh, rf) == (194, 255)
    want = [(2, (98, 127)), (1, (99, 126)), (2, (50, 63)), (1, (51, 62)), (1, (52, 61)), (2, (27, 30))]
    for stride, zn in want:
        rf = RR.rf_conv3x3(rf, stride)
        oh = (oh - 1) // stride + 1
        assert RR.zone(p0, H, oh, rf) == zn
    assert RR.zone(p0, H, oh, RR.rf_conv3x3(rf, 1)) is None  # block 7: nothing left


@pytest.mark.parametrize("OH,R", [(33, 2), (33, 5), (33, 11), (33, 33), (17, 3), (129, 8)])
def test_band_segments_cover_the_computed_rows_once(OH, R):
    nby = -(-OH // R)
    for zn in [None, (21, 31), (2, 31), (0, OH), (OH - 2, OH), (5, 7)]:
        if zn is not None and zn[1] > OH:
            continue
        rows = []
        for by in range(nby):
            segs = RR.band_segments(zn, OH, R, by)
            assert len(segs) <= 2 and sum(y1 - y0 for y0, y1 in segs) <= R
            for y0, y1 in segs:
                rows += list(range(y0, y1))
        want = [o for o in range(OH) if zn is None or not zn[0] < o < zn[1]]
        assert rows == want, (zn, rows)


def test_switch(monkeypatch):
    monkeypatch.delenv("SSA_ROW_REPEAT", raising=False)
    assert RR.enabled()
    monkeypatch.setenv("SSA_ROW_REPEAT", "0")
    assert not RR.enabled()


_MODEL = []


def _front_launches(monkeypatch, cam, picks, flag, B=32, S=513):
    """Builds the plan on the CPU, sets ``picks`` and calls the front ops with the launch
    wrappers replaced by recorders: {choice name: row repeat on?} of stem_band / fused_ir_slice."""
    from semantic_segmentation_server_amd import config as C
    from semantic_segmentation_server_amd.models import hip_model as HM
    from semantic_segmentation_server_amd.models.deeplab import build_model
    from semantic_segmentation_server_amd.models.plan import Choice, HipPlanModel
    monkeypatch.setattr(HipPlanModel, "_launch", staticmethod(lambda ops, args: None))
    monkeypatch.setattr(HipPlanModel, "_autotune", lambda self, *a: setattr(self, "choices", {}))
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a: None)
    if flag is None:
        monkeypatch.delenv("SSA_ROW_REPEAT", raising=False)
    else:
        monkeypatch.setenv("SSA_ROW_REPEAT", flag)
    seen = []
    monkeypatch.setattr(HM.K, "stem_band", lambda *a, **kw: seen.append(bool(kw.get("row_repeat"))))
    monkeypatch.setattr(HM.FB, "fused_ir_slice", lambda *a, **kw: seen.append(kw.get("lut_y") is not None))
    if not _MODEL:
        _MODEL.append(build_model("mnv2", 21, calibrate_hw=65))
    hm = HM.HipDeepLab(_MODEL[0], torch.device("cpu"), C.Config(backend="hip", batch=B, input_size=S, graph=False))
    ops, _ = hm._plan(B, cam[1], cam[0])
    out = {}
    for op in ops:
        if isinstance(op, Choice) and op.name in picks:
            op.pick = [n for n, _ in op.variants].index(picks[op.name])
            del seen[:]
            op("frames", "lx", "ly")
            out[op.name] = seen[0]
    return out


def test_plan_policy_at_the_headline_shape(monkeypatch):
    """Default: the repeat is on where a band of the picked launch gets shorter at the plan's
    camera, in the stem and the stride-2 slice blocks; ``all``: everywhere; ``0``: nowhere;
    a square camera (no pad): nowhere, so no launch pays for the LUT scan."""
    import json
    from semantic_segmentation_server_amd.models.hip_model import TUNE_FILE_DEFAULT
    saved = json.load(open(TUNE_FILE_DEFAULT))["mnv2:B=32:cam=640x480:in=513"]
    picks = {n: saved[n] for n in ("stem+block0", "block1", "block2", "block3", "block6")}
    assert picks["stem+block0"].startswith("stem_band") and picks["block6"].startswith("slice")
    assert _front_launches(monkeypatch, (640, 480), picks, None) == {
        "stem+block0": True, "block1": True, "block2": False, "block3": True, "block6": False}
    assert set(_front_launches(monkeypatch, (640, 480), picks, "all").values()) == {True}
    assert set(_front_launches(monkeypatch, (640, 480), picks, "0").values()) == {False}
    assert set(_front_launches(monkeypatch, (513, 513), picks, None).values()) == {False}
