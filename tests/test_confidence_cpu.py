"""--serve_confidence without a GPU: the definition (ops/reference_ops.upsample_confidence)
against float64, the 7-word region format, its transport (hub, worker channel, pipeline) and the
v2 GetClassRegions fields, the flags, and a CPU producer end to end."""
import os

import grpc
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from semantic_segmentation_server_amd import config as C
from semantic_segmentation_server_amd.api import proto as P
from semantic_segmentation_server_amd.api import service as S
from semantic_segmentation_server_amd.ops import reference_ops as R
from semantic_segmentation_server_amd.postprocess import regions as RG
from semantic_segmentation_server_amd.runtime.results import ResultHub

# the shapes of the device kernel's test (tests/test_confidence_gpu.py)
CASES = [(2, 9, 9, 65, 65, 21), (2, 9, 9, 65, 65, 19), (2, 33, 33, 257, 257, 30), (2, 5, 5, 40, 40, 40),
         (3, 9, 13, 65, 97, 21)]


def _logits(B, h, w, K, field):
    g = torch.Generator().manual_seed(7)
    ldk = (K + 7) // 8 * 8
    if field == "noise":
        logits = torch.randn(B, h, w, ldk, generator=g).to(torch.bfloat16)
    else:
        coarse = torch.randn(B, ldk, 4, 4, generator=g) * 4
        logits = F.interpolate(coarse, size=(h, w), mode="bilinear", align_corners=True) \
            .permute(0, 2, 3, 1).contiguous().to(torch.bfloat16)
    return logits[..., :K].permute(0, 3, 1, 2).contiguous()  # NCHW, the real classes


@pytest.mark.parametrize("field", ["noise", "smooth"])
@pytest.mark.parametrize("B,h,w,H,W,K", CASES)
def test_definition_against_float64(B, h, w, H, W, K, field):
    """The bounds of the device test: |conf - 255 p64| <= 0.5 + 0.01 at every pixel; the label is
    the float64 argmax wherever the float64 top-two margin exceeds 1e-4, and the inputs leave at
    most 0.2 % of the map below that margin."""
    x = _logits(B, h, w, K, field)
    assert x.float().abs().max() < 32
    labels, conf = R.upsample_confidence(x.float(), H, W)
    assert labels.dtype == conf.dtype == torch.uint8 and labels.shape == conf.shape == (B, H, W)
    u = F.interpolate(x.double(), size=(H, W), mode="bilinear", align_corners=True)
    c64 = 255.0 * torch.softmax(u, 1).amax(1)
    top2 = u.topk(2, dim=1).values
    decided = (top2[:, 0] - top2[:, 1]) > 1e-4
    assert (conf.double() - c64).abs().max() <= 0.5 + 0.01
    assert 1.0 - decided.double().mean().item() <= 0.002
    assert torch.equal(labels.long()[decided], u.argmax(1)[decided])
    assert torch.equal(labels, R.upsample_argmax(x.float(), H, W))
    assert int(conf.min()) >= int(np.floor(255.0 / K + 0.5 - 0.01))  # p >= 1 / K: 12 .. 255 at K = 21


def test_definition_extremes():
    x = torch.zeros((1, 21, 2, 2))
    _, conf = R.upsample_confidence(x, 5, 5)
    assert (conf == 12).all()  # floor(255 / 21 + 0.5)
    x[:, 7] = 40.0
    labels, conf = R.upsample_confidence(x, 5, 5)
    assert (conf == 255).all() and (labels == 7).all()


# ---- the format ---------------------------------------------------------------------------------

def _frame(seed, H=24, W=30):
    rng = np.random.default_rng(seed)
    coarse = rng.integers(0, 5, (H // 4 + 1, W // 4 + 1)).astype(np.uint8)
    lab = np.repeat(np.repeat(coarse, 4, 0), 4, 1)[:H, :W].copy()
    return lab, rng.integers(0, 256, (H, W)).astype(np.uint8)


def test_encode_decode_round_trip_and_sum_conf_by_brute_force():
    lab, conf = _frame(1)
    ch, cw, K = 21, 27, 32
    w7 = RG.encode(lab, cw, ch, [1, 2, 3, 4], 2, K, conf=conf)
    w6 = RG.encode(lab, cw, ch, [1, 2, 3, 4], 2, K)
    assert w7.shape == (4 + 7 * K,) and w6.shape == (4 + 6 * K,) and np.array_equal(w7[:4], w6[:4])
    t7, t6 = RG.decode(w7, conf=True), RG.decode(w6)
    assert len(t7) == len(t6) == int(w6[0]) > 3
    names = [n for n in RG.REGION_DTYPE.names if n != "sum_conf"]
    assert all(np.array_equal(t7[n], t6[n]) for n in names) and (t6["sum_conf"] == 0).all()
    assert RG.used_words(w7, conf=True) == 4 + 7 * len(t7) and RG.used_words(w6) == 4 + 6 * len(t6)
    assert np.array_equal(RG.pack(t7, conf=True).reshape(-1), w7[4:4 + 7 * len(t7)])
    roots = RG.label_components(lab[:ch, :cw], RG.class_mask([1, 2, 3, 4]))
    for t in t7:
        on = roots == int(t["root"])
        assert int(on.sum()) == int(t["pixels"])
        assert int(t["sum_conf"]) == int(conf[:ch, :cw][on].astype(np.int64).sum())
    full = RG.decode(RG.encode(np.full((9, 9), 3, np.uint8), 9, 9, [3], 1, 2,
                               conf=np.full((9, 9), 255, np.uint8)), conf=True)
    assert full["sum_conf"].tolist() == [255 * 81]
    with pytest.raises(ValueError):
        RG.encode(lab, cw, ch, [1], 2, K, conf=conf[:, :-1])
    with pytest.raises(ValueError):
        RG.encode(lab, cw, ch, [1], 2, K, conf=conf, out=np.zeros(4 + 6 * K, np.uint32))


def test_cut_off_keeps_the_true_count_with_seven_words():
    lab, conf = _frame(2)
    w = RG.encode(lab, 30, 24, [1, 2, 3, 4], 1, 3, conf=conf)
    every = RG.region_table(lab, 30, 24, [1, 2, 3, 4], 1, conf=conf)
    assert w[0] == len(every) > 3 and RG.used_words(w, conf=True) == 4 + 21
    assert np.array_equal(RG.decode(w, conf=True), every[:3])


# ---- transport ------------------------------------------------------------------------------------

def _rows(frames, K, conf=True):
    return np.stack([RG.encode(l, l.shape[1], l.shape[0], range(1, 21), 1, K, conf=c if conf else None)
                     for l, c in frames])


def test_hub_records_whether_an_item_has_confidence():
    frames = [_frame(3), _frame(4)]
    hub = ResultHub(2)
    r7, r6 = _rows(frames, 4), _rows(frames, 4, conf=False)
    hub.push_regions(r7.view(np.int32), np.array([[10, 0, 1.0], [11, 1, 1.5]]), conf=True)
    a = hub.regions(0)
    assert a.conf and np.array_equal(a.words, r7[0][:RG.used_words(r7[0], conf=True)])
    assert len(a.words) == 4 + 7 * 4
    hub.push_regions(r6[1:], np.array([[12, 1, 2.0]]))  # a producer without the flag
    b = hub.regions(1)
    assert not b.conf and b.frame_id == 12 and len(b.words) == 4 + 6 * 4
    hub.put_regions(1, 13, 3.0, r7[1], conf=True)
    assert hub.regions(1).conf and hub.regions(0).frame_id == 10


def test_word_channel_unit_seven_round_trip():
    from semantic_segmentation_server_amd.runtime.supervisor import _RingHub, _WordChannel
    frames = [_frame(5), _frame(6), _frame(7)]
    rows = _rows(frames, 4)
    ch = _WordChannel(streams=2, cap=4, first=4, unit=7)
    try:
        peer = _WordChannel(name=ch.name)
        assert (peer.S, peer.cap, peer.first, peer.unit) == (2, 4, 4, 7) and ch.pull() == []
        hub = _RingHub(None, None, peer)
        hub.push_regions(rows[:2], np.array([[7, 4, 1.0], [8, 4, 2.0]]), conf=True)
        hub.push_regions(rows[2:], np.array([[3, 5, 0.5]]), conf=True)
        got = ch.pull()
        assert [(s, f, t) for s, f, t, _ in got] == [(4, 8, 2.0), (5, 3, 0.5)]
        for (_, _, _, w), want in zip(got, (rows[1], rows[2])):
            assert len(w) == 4 + 7 * 4 and np.array_equal(w, want[:RG.used_words(want, conf=True)])
        assert ch.pull() == []
        peer.write(4, 9, 3.0, rows[0])
        ((s, f, _, w),) = ch.pull()
        assert (s, f) == (4, 9) and np.array_equal(RG.decode(w, conf=True), RG.decode(rows[0], conf=True))
        peer.close()
    finally:
        ch.close()


# ---- RPC ------------------------------------------------------------------------------------------

class _Ctx:
    code = None

    def set_code(self, c):
        self.code = c

    def set_details(self, d):
        self.details = d


def _labelled():
    lab = np.zeros((6, 8), np.uint8)
    lab[1:4, 2:7] = 15   # 15 pixels
    lab[5, 0:2] = 7      # 2 pixels
    lab[0, 7] = 3        # 1 pixel
    conf = (np.arange(48, dtype=np.int64).reshape(6, 8) * 5 + 13).astype(np.uint8)
    return lab, conf


def test_handler_confidence_comes_from_the_integer_words():
    lab, conf = _labelled()
    rows = _rows([(lab, conf)], 2)  # K = 2: the third region is cut off
    hub = ResultHub(1)
    hub.push_regions(rows, np.array([[4, 0, 9.5]]), conf=True)
    sv = S.SemanticSegmentationV2Servicer(hub, {15: "person", 7: "car"}, serve_regions=True, model_size=(16, 8))
    m = sv.GetClassRegions(P.RegionRequest(stream_id=0), _Ctx())
    assert m.has_confidence and (m.total_regions, m.truncated) == (3, True)
    a, b = m.regions
    sa, sb = int(conf[1:4, 2:7].astype(np.int64).sum()), int(conf[5, 0:2].astype(np.int64).sum())
    assert (a.pixels, b.pixels) == (15, 2)
    assert a.confidence == np.float32(sa / (255 * 15)) and b.confidence == np.float32(sb / (255 * 2))
    assert 0 < a.confidence <= 1
    # the other fields are those of the 6-word rows
    hub6 = ResultHub(1)
    hub6.push_regions(_rows([(lab, conf)], 2, conf=False), np.array([[4, 0, 9.5]]))
    sv6 = S.SemanticSegmentationV2Servicer(hub6, {15: "person", 7: "car"}, serve_regions=True, model_size=(16, 8))
    m6 = sv6.GetClassRegions(P.RegionRequest(stream_id=0), _Ctx())
    assert not m6.has_confidence and [r.confidence for r in m6.regions] == [0.0, 0.0]
    for r, r6 in zip(m.regions, m6.regions):
        r.confidence = 0.0
        assert r == r6
    one = sv.GetClassRegions(P.RegionRequest(stream_id=0, max_regions=1), _Ctx())  # max_regions still cuts
    assert len(one.regions) == 1 and one.has_confidence and one.truncated and one.total_regions == 3
    assert one.regions[0].confidence == np.float32(sa / (255 * 15))


def test_proto_lists_the_new_fields_and_v1_has_none():
    v2 = {m.name: {f.name: (f.number, f.type) for f in m.field} for m in P.v2_file_descriptor().message_type}
    from google.protobuf.descriptor_pb2 import FieldDescriptorProto as F_
    assert v2["ClassRegion"]["confidence"] == (11, F_.TYPE_FLOAT)
    assert v2["ClassRegions"]["has_confidence"] == (11, F_.TYPE_BOOL)
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                        "semantic_segmentation_server_amd", "api", "sem_seg_server_v2.proto")
    with open(path) as f:
        text = f.read()
    assert "float confidence = 11;" in text and "bool has_confidence = 11;" in text
    for m in P.v1_file_descriptor().message_type:
        assert not any("confidence" in f.name for f in m.field)


def test_client_prints_a_confidence_column(capsys):
    from semantic_segmentation_server_amd import client
    r = P.ClassRegion(label="person", class_id=15, pixels=15, confidence=0.75)
    client.print_regions(P.ClassRegions(regions=[r], total_regions=1, has_confidence=True))
    assert "conf 0.750" in capsys.readouterr().out
    client.print_regions(P.ClassRegions(regions=[r], total_regions=1))
    assert "conf" not in capsys.readouterr().out


# ---- flags and serving on the CPU -----------------------------------------------------------------

def _cfg(**kw):
    base = dict(backend="torch", device="cpu", input_size=65, batch=1, port=0, host="127.0.0.1",
                min_area_ratio=0.0005, fps_limit=200.0, log_level="WARNING")
    base.update(kw)
    return C.Config(**base)


def test_flag_is_off_by_default_and_refused_without_regions():
    assert C.parse([]).serve_confidence is False
    cfg = C.parse(["--serve_regions", "--serve_confidence"])
    assert cfg.serve_regions and cfg.serve_confidence
    with pytest.raises(ValueError) as e:
        C.parse(["--serve_confidence"])
    assert "--serve_confidence" in str(e.value) and "--serve_regions" in str(e.value)
    with pytest.raises(ValueError, match="--serve_regions"):
        C.Config(serve_confidence=True)


def test_engine_step_on_cpu_uses_the_definition():
    from semantic_segmentation_server_amd.runtime.engine import Engine
    from semantic_segmentation_server_amd.runtime.sources import SyntheticSource
    eng = Engine(_cfg(serve_regions=True, serve_confidence=True, batch=2))
    off = Engine(_cfg(serve_regions=True, batch=2))
    f, _, _ = SyntheticSource(160, 120, pool=2, seed=3).read_batch(2)
    recs = eng.step(f, [0, 1], [0.0, 0.0], [0, 1])
    recs_off = off.step(f, [0, 1], [0.0, 0.0], [0, 1])
    with torch.no_grad():
        x = R.preprocess(torch.from_numpy(f), eng.lut_x, eng.lut_y)
        lab, conf = R.upsample_confidence(eng.model(x), 65, 65)
    assert torch.equal(eng.conf_plane, conf) and off.conf_plane is None
    assert eng.regions.shape == (2, 4 + 7 * 64) and off.regions.shape == (2, 4 + 6 * 64)
    for b in range(2):
        want = RG.encode(lab[b].numpy(), eng.crop_w, eng.crop_h, RG.default_classes(21),
                         eng.region_min_pixels, 64, conf=conf[b].numpy())
        assert np.array_equal(eng.regions[b], want)
        t7, t6 = RG.decode(eng.regions[b], conf=True), RG.decode(off.regions[b])
        assert np.array_equal(t7[["label", "root", "pixels"]], t6[["label", "root", "pixels"]])
    assert recs.tobytes() == recs_off.tobytes()


def test_cpu_producer_pushes_seven_word_rows_that_the_rpc_decodes():
    from semantic_segmentation_server_amd.server import Server
    srv = Server(_cfg(serve_regions=True, serve_confidence=True, fps_limit=None,
                      region_min_area_ratio=0.001), max_steps=3).start()
    try:
        srv.producer.join(timeout=120)
        assert srv.producer.steps == 3 and srv.producer.error is None
        with grpc.insecure_channel(f"127.0.0.1:{srv.port}") as ch:
            m = S.SemanticSegmentationV2Stub(ch).GetClassRegions(P.RegionRequest(stream_id=0))
        stored = srv.hub.regions(0)
        assert stored.conf and m.has_confidence and m.frame_id == 2
        tab = RG.decode(stored.words, conf=True)
        assert len(stored.words) == RG.used_words(stored.words, 64, conf=True)
        assert len(m.regions) == len(tab) > 0 and m.total_regions == int(stored.words[0])
        for r, t in zip(m.regions, tab):
            assert (r.class_id, r.pixels) == (int(t["label"]), int(t["pixels"]))
            assert r.confidence == np.float32(int(t["sum_conf"]) / (255 * int(t["pixels"])))
            assert 12 / 255 <= r.confidence <= 1.0
    finally:
        srv.stop(0)
