"""Zone occupancy (postprocess/zones.py) without a GPU: the exact-integer rasteriser, the zone
file's refusals, the statistics and their limits, and the layers that carry the words on the
CPU: config, engine, hub, supervisor channel, servicer, RPC, server, client.
"""
import json
import time
from concurrent import futures

import grpc
import numpy as np
import pytest
import torch

from semantic_segmentation_server_amd import config as C
from semantic_segmentation_server_amd.api import proto as P
from semantic_segmentation_server_amd.api import service as S
from semantic_segmentation_server_amd.postprocess import zones as ZN
from semantic_segmentation_server_amd.runtime.results import ResultHub

CROPS = [(513, 384), (7, 5), (1, 1)]


def _rect(name, x0, y0, x1, y1):
    return ZN.parse({"zones": [{"name": name, "rect": [x0, y0, x1, y1]}]})[0]


def _poly(name, pts):
    return ZN.Zone(name, tuple((float(x), float(y)) for x, y in pts))


def _bit(plane, z):
    return ((plane >> np.uint32(z - 1)) & np.uint32(1)).astype(bool)


# ---- the rasteriser -------------------------------------------------------------------------

@pytest.mark.parametrize("crop", CROPS)
@pytest.mark.parametrize("split", [0.5, 1 / 3, 0.37, 0.0, 1.0])
def test_two_rectangles_sharing_an_edge_partition_the_crop(crop, split):
    cw, ch = crop
    for zl in ([_rect("l", 0, 0, split, 1), _rect("r", split, 0, 1, 1)],
               [_rect("t", 0, 0, 1, split), _rect("b", 0, split, 1, 1)]):
        p = ZN.rasterize(zl, cw, ch, warn=False)
        assert p.shape == (ch, cw) and p.dtype == np.uint32 and p.flags["C_CONTIGUOUS"]
        assert (_bit(p, 1) ^ _bit(p, 2)).all()  # no pixel lost, none doubled


@pytest.mark.parametrize("crop", CROPS)
def test_three_polygons_sharing_a_vertex_partition_the_crop(crop):
    cw, ch = crop
    c = (0.43, 0.61)  # the shared vertex; the three polygons tile the unit square around it
    zl = [_poly("a", [c, (0, 0), (1, 0), (1, 0.3)]),
          _poly("b", [c, (1, 0.3), (1, 1), (0, 1), (0, 0.8)]),
          _poly("c", [c, (0, 0.8), (0, 0)])]
    p = ZN.rasterize(zl, cw, ch, warn=False)
    count = _bit(p, 1).astype(int) + _bit(p, 2) + _bit(p, 3)
    assert (count == 1).all()


def test_vertex_order_and_start_do_not_change_the_plane():
    pts = [(0.1, 0.15), (0.85, 0.05), (0.95, 0.7), (0.5, 0.45), (0.2, 0.9)]
    base = ZN.rasterize([_poly("p", pts)], 129, 97)
    assert 0 < _bit(base, 1).sum() < 129 * 97
    for k in range(len(pts)):
        rot = pts[k:] + pts[:k]
        assert np.array_equal(ZN.rasterize([_poly("p", rot)], 129, 97), base)
        assert np.array_equal(ZN.rasterize([_poly("p", rot[::-1])], 129, 97), base)


def test_self_intersecting_star_follows_even_odd():
    # a pentagram: the inner pentagon is wound twice, so even-odd leaves it out
    ang = [np.pi / 2 + 2 * np.pi * k * 2 / 5 for k in range(5)]
    pts = [(0.5 + 0.45 * np.cos(a), 0.5 - 0.45 * np.sin(a)) for a in ang]
    m = _bit(ZN.rasterize([_poly("star", pts)], 201, 201), 1)
    assert not m[100, 100]                    # the centre
    assert m[100 - 60, 100]                   # inside the top point
    assert not m[0, 0] and not m[200, 200]    # outside
    tip = (0.5 + 0.3 * np.cos(ang[1]), 0.5 - 0.3 * np.sin(ang[1]))
    assert m[int(tip[1] * 201), int(tip[0] * 201)]


def test_polygon_outside_the_frame_is_an_empty_zone(caplog):
    zl = [_poly("out", [(1.5, 1.5), (2.5, 1.5), (2.0, 2.5)]), _rect("neg", -3, -3, -0.01, -0.01)]
    with caplog.at_level("WARNING"):
        p = ZN.rasterize(zl, 65, 48)
    assert not p.any()
    assert sum("covers no pixel" in r.getMessage() for r in caplog.records) == 2


def test_rect_equals_its_four_vertex_polygon():
    r = _rect("r", 0.12, 0.2, 0.77, 0.93)
    q = _poly("q", [(0.12, 0.2), (0.77, 0.2), (0.77, 0.93), (0.12, 0.93)])
    assert r.polygon == q.polygon
    for cw, ch in CROPS + [(64, 33)]:
        assert np.array_equal(ZN.rasterize([r], cw, ch, warn=False), ZN.rasterize([q], cw, ch, warn=False))
    # pixel centres decide: the rectangle 0.25 .. 0.75 of an 8 x 4 crop is columns 2 .. 5, rows 1 .. 2
    m = _bit(ZN.rasterize([_rect("h", 0.25, 0.25, 0.75, 0.75)], 8, 4), 1)
    want = np.zeros((4, 8), bool)
    want[1:3, 2:6] = True
    assert np.array_equal(m, want)


def test_zone_32_lands_in_bit_31():
    zl = [_rect(f"z{k}", 2, 2, 3, 3) for k in range(31)] + [_rect("last", 0, 0, 1, 1)]
    p = ZN.rasterize(zl, 9, 7, warn=False)
    assert (p == 0x80000000).all() and ZN.rows_of(p) == 33


# ---- the zone file ---------------------------------------------------------------------------

def _load(tmp_path, obj):
    f = tmp_path / "zones.json"
    f.write_text(json.dumps(obj))
    return ZN.load(str(f))


def test_file_is_read(tmp_path):
    zl = _load(tmp_path, {"zones": [{"name": "door", "polygon": [[0, 0], [1, 0], [0.5, 1.2]]},
                                    {"name": "bay", "rect": [0.1, 0.2, 0.3, 0.4]}]})
    assert ZN.names(zl) == ["frame", "door", "bay"] and len(zl[0].polygon) == 3 and len(zl[1].polygon) == 4
    assert _load(tmp_path, {"zones": []}) == []


@pytest.mark.parametrize("zones, needle", [
    ([{"name": f"z{k}", "rect": [0, 0, 1, 1]} for k in range(33)], "z32"),
    ([{"name": "a", "rect": [0, 0, 1, 1]}, {"name": "a", "rect": [0, 0, 1, 1]}], "'a'"),
    ([{"name": "frame", "rect": [0, 0, 1, 1]}], "'frame'"),
    ([{"name": "thin", "polygon": [[0, 0], [1, 1]]}], "'thin'"),
    ([{"name": "nan", "polygon": [[0, 0], [1, "x"], [1, 1]]}], "'nan'"),
    ([{"name": "", "rect": [0, 0, 1, 1]}], "zone 1"),
    ([{"name": "both", "rect": [0, 0, 1, 1], "polygon": [[0, 0], [1, 0], [1, 1]]}], "'both'"),
    ([{"name": "far", "rect": [0, 0, 1e9, 1]}], "'far'"),
])
def test_file_errors_name_the_file_and_the_zone(tmp_path, zones, needle):
    with pytest.raises(ValueError) as e:
        _load(tmp_path, {"zones": zones})
    assert "zones.json" in str(e.value) and needle in str(e.value)


def test_unreadable_file_is_named(tmp_path):
    with pytest.raises(ValueError, match="nothing.json"):
        ZN.load(str(tmp_path / "nothing.json"))
    (tmp_path / "bad.json").write_text("{")
    with pytest.raises(ValueError, match="bad.json"):
        ZN.load(str(tmp_path / "bad.json"))


# ---- statistics ------------------------------------------------------------------------------

def test_encode_by_hand_and_decode_round_trip():
    lab = np.array([[0, 0, 1, 9],
                    [2, 2, 1, 9],
                    [9, 9, 9, 9]], np.uint8)  # crop 3 x 2 inside a 4 x 3 map
    plane = np.array([[1, 3, 2],
                      [0, 1, 2]], np.uint32)
    conf = np.arange(12, dtype=np.uint8).reshape(3, 4) + 10
    w = ZN.encode(lab, plane, 3, 2, 3, conf=conf, rows=3)
    assert w.dtype == np.uint32 and len(w) == 4 + 2 * 9 == ZN.frame_words(3, 3, True)
    assert w[:4].tolist() == [3, 6, 3, 2]
    t = ZN.decode(w, conf=True)
    assert (t.rows, t.n, t.crop_w, t.crop_h) == (3, 6, 3, 2)
    assert t.pixels.tolist() == [[2, 2, 2], [2, 0, 1], [1, 2, 0]]
    assert t.sum_conf.tolist() == [[10 + 11, 12 + 16, 14 + 15], [10 + 11, 0, 15], [11, 12 + 16, 0]]
    plain = ZN.encode(lab, plane, 3, 2, 3, rows=3)
    assert np.array_equal(plain, w[:4 + 9]) and ZN.decode(plain).sum_conf is None
    out = np.full(4 + 18, 0xDEADBEEF, np.uint32)  # every word is written, zeros included
    assert ZN.encode(lab, plane, 3, 2, 3, conf=conf, rows=3, out=out) is out and np.array_equal(out, w)
    assert ZN.rows_of(plane) == 3 and np.array_equal(ZN.encode(lab, plane, 3, 2, 3), plain)
    assert ZN.encode(lab, None, 3, 2, 3).tolist() == [1, 6, 3, 2, 2, 2, 2]
    with pytest.raises(ValueError):
        ZN.encode(lab, None, 3, 2, 3, rows=2)
    with pytest.raises(ValueError):
        ZN.decode(w[:-1], conf=True)


def test_frame_row_sums_to_n_unless_labels_pass_the_classes():
    rng = np.random.default_rng(0)
    lab = rng.integers(0, 21, (40, 50)).astype(np.uint8)
    plane = rng.integers(0, 16, (37, 45)).astype(np.uint32)
    t = ZN.decode(ZN.encode(lab, plane, 45, 37, 21, rows=5))
    assert t.pixels[0].sum() == 45 * 37
    for z in range(1, 5):
        assert t.pixels[z].sum() == _bit(plane, z).sum()
    t5 = ZN.decode(ZN.encode(lab, plane, 45, 37, 5, rows=5))
    inside = lab[:37, :45] < 5
    assert t5.pixels[0].sum() == inside.sum() < 45 * 37
    assert np.array_equal(t5.pixels, t.pixels[:, :5])
    lab[:] = 200
    assert not ZN.encode(lab, plane, 45, 37, 21, rows=5)[4:].any()  # labels >= C count nowhere


def test_check_geometry_at_each_limit_and_one_past():
    ZN.check_geometry(4096, 4095, 32, 21)          # N = 2^24 - 4096
    ZN.check_geometry(1, (1 << 24) - 1, 0, 1)      # N = 2^24 - 1
    with pytest.raises(ValueError, match="--serve_zones"):
        ZN.check_geometry(4096, 4096, 0, 1)        # N = 2^24
    with pytest.raises(ValueError, match="--serve_zones"):
        ZN.check_geometry(513, 513, 33, 21)        # Z = 33
    ZN.check_geometry(513, 513, 32, 124)           # 33 * 124 = 4092
    with pytest.raises(ValueError, match="--serve_zones"):
        ZN.check_geometry(513, 513, 32, 125)       # 33 * 125 = 4125 > ZONE_COUNTERS
    ZN.check_geometry(513, 513, 15, 256)           # 16 * 256 = 4096
    with pytest.raises(ValueError, match="15 zones"):
        ZN.check_geometry(513, 513, 16, 256)
    with pytest.raises(ValueError, match="--serve_zones"):
        ZN.check_geometry(513, 513, 0, 257)        # C = 257
    with pytest.raises(ValueError, match="--serve_zones"):
        ZN.check_geometry(513, 513, 0, 0)
    with pytest.raises(ValueError, match="--serve_zones"):
        ZN.check_geometry(0, 5, 0, 21)
    assert ZN.ZONE_COUNTERS == 4096 and ZN.MAX_ZONES == 32 and ZN.MAX_CLASSES == 256


# ---- config ----------------------------------------------------------------------------------

def test_cli_flags_and_refusals():
    d = C.parse([])
    assert (d.serve_zones, d.zones) == (False, None)
    cfg = C.parse(["--serve_zones", "--zones", "z.json"])
    assert (cfg.serve_zones, cfg.zones) == (True, "z.json")
    assert C.parse(["--serve_zones"]).zones is None  # the frame row alone
    cfg = C.parse(["--serve_confidence", "--serve_zones"])
    assert cfg.serve_confidence and cfg.serve_zones and not cfg.serve_regions
    with pytest.raises(ValueError) as e:
        C.parse(["--zones", "z.json"])
    assert "--zones" in str(e.value) and "--serve_zones" in str(e.value)
    with pytest.raises(ValueError) as e:
        C.parse(["--serve_confidence"])
    assert "--serve_confidence" in str(e.value) and "--serve_regions" in str(e.value)


# ---- engine on the CPU -------------------------------------------------------------------------

ZONES = {"zones": [{"name": "left", "rect": [0.0, 0.0, 0.5, 1.0]},
                   {"name": "right", "rect": [0.5, 0.0, 1.0, 1.0]},
                   {"name": "tri", "polygon": [[0.1, 0.1], [0.9, 0.25], [0.4, 0.95]]}]}


@pytest.fixture(scope="module")
def zone_file(tmp_path_factory):
    p = tmp_path_factory.mktemp("zones") / "zones.json"
    p.write_text(json.dumps(ZONES))
    return str(p)


def _cfg(**kw):
    base = dict(backend="torch", device="cpu", input_size=65, batch=1, port=0, host="127.0.0.1",
                min_area_ratio=0.0005, fps_limit=200.0, log_level="WARNING")
    base.update(kw)
    return C.Config(**base)


@pytest.mark.parametrize("conf", [False, True])
def test_engine_step_zones_on_cpu(conf, zone_file):
    from semantic_segmentation_server_amd.runtime.engine import Engine
    from semantic_segmentation_server_amd.runtime.sources import SyntheticSource
    eng = Engine(_cfg(serve_zones=True, zones=zone_file, serve_confidence=conf, batch=2))
    f, _, _ = SyntheticSource(160, 120, pool=2, seed=3).read_batch(2)
    recs = eng.step(f, [0, 1], [0.0, 0.0], [0, 1])
    with torch.no_grad():
        lab, cf = eng._infer(torch.from_numpy(f))
    assert eng.zone_rows == 4 and eng.zones.shape == (2, 4 + 4 * 21 * (2 if conf else 1))
    assert eng.zones.dtype == np.uint32 and np.array_equal(eng.zone_plane, ZN.rasterize(ZN.load(zone_file), eng.crop_w, eng.crop_h))
    for b in range(2):
        want = ZN.encode(lab[b].numpy(), eng.zone_plane, eng.crop_w, eng.crop_h, 21, rows=4,
                         conf=cf[b].numpy() if conf else None)
        assert np.array_equal(eng.zones[b], want)
        t = ZN.decode(eng.zones[b], conf=conf)
        assert t.pixels[0].sum() == eng.crop_w * eng.crop_h == t.pixels[1].sum() + t.pixels[2].sum()
    off = Engine(_cfg(batch=2))
    recs_off = off.step(f, [0, 1], [0.0, 0.0], [0, 1])
    assert off.zones is None and off.zone_rows == 0 and recs.tobytes() == recs_off.tobytes()
    # without --zones: the frame row alone
    alone = Engine(_cfg(serve_zones=True, batch=2))
    alone.step(f, [0, 1], [0.0, 0.0], [0, 1])
    assert alone.zone_rows == 1 and alone.zones.shape == (2, 4 + 21)
    assert np.array_equal(alone.zones[0], ZN.encode(lab[0].numpy(), None, eng.crop_w, eng.crop_h, 21))


def test_engine_checks_the_zones_when_it_is_built(tmp_path):
    from semantic_segmentation_server_amd.runtime.engine import Engine
    bad = tmp_path / "bad.json"
    bad.write_text(json.dumps({"zones": [{"name": "frame", "rect": [0, 0, 1, 1]}]}))
    with pytest.raises(ValueError, match="bad.json"):
        Engine(_cfg(serve_zones=True, zones=str(bad)))
    many = tmp_path / "many.json"
    many.write_text(json.dumps({"zones": [{"name": f"z{k}", "rect": [0, 0, 1, 1]} for k in range(16)]}))
    with pytest.raises(ValueError, match="--serve_zones"):
        Engine(_cfg(serve_zones=True, zones=str(many), num_classes=256))  # 17 * 256 counters


# ---- hub, channel, servicer ------------------------------------------------------------------

def _rows(R, C, conf, fill):
    rows = np.zeros((len(fill), ZN.frame_words(R, C, conf)), np.uint32)
    for i, v in enumerate(fill):
        rows[i, :4] = (R, 12, 4, 3)
        rows[i, 4:] = v
    return rows


def test_hub_keeps_the_latest_per_stream():
    hub = ResultHub(2)
    assert hub.zones(0) is None
    rows = _rows(2, 3, False, [1, 2, 3])
    hub.push_zones(rows.view(np.int32), np.array([[10, 0, 1.0], [11, 1, 2.0], [12, 0, 3.0]]))
    z0, z1 = hub.zones(0), hub.zones(1)
    assert (z0.frame_id, z0.ts, z0.conf) == (12, 3.0, False) and np.array_equal(z0.words, rows[2])
    assert (z1.frame_id, z1.ts) == (11, 2.0) and np.array_equal(z1.words, rows[1])
    rows[2] = 0
    assert hub.zones(0).words[4] == 3  # the hub's own copy
    hub.push_zones(_rows(2, 3, True, [7]), np.array([[13, 0, 4.0]]), conf=True)
    z0 = hub.zones(0)
    assert z0.frame_id == 13 and z0.conf and len(z0.words) == 4 + 12 and hub.zones(1).frame_id == 11


def test_word_channel_carries_whole_frames():
    from semantic_segmentation_server_amd.runtime.supervisor import _RingHub, _WordChannel
    ch = _WordChannel(2, 3, first=4, unit=5 * 2)  # R = 3 rows of C = 5 classes with confidence
    try:
        rows = _rows(3, 5, True, [9, 8])
        _RingHub(None, zones=ch).push_zones(rows, np.array([[20, 4, 1.5], [21, 5, 2.5]]), conf=True)
        got = {s: (fid, ts, w) for s, fid, ts, w in ch.pull()}
        assert set(got) == {4, 5} and got[4][:2] == (20, 1.5) and got[5][:2] == (21, 2.5)
        assert np.array_equal(got[4][2], rows[0]) and np.array_equal(got[5][2], rows[1])
        assert ch.pull() == []
    finally:
        ch.close()


class _Ctx:
    code = None

    def set_code(self, c):
        self.code = c

    def set_details(self, d):
        self.details = d


def test_status_codes():
    hub = ResultHub(1)
    on = S.SemanticSegmentationV2Servicer(hub, {}, zone_names=["frame", "a"], model_size=(9, 9))
    off = S.SemanticSegmentationV2Servicer(hub, {}, model_size=(9, 9))
    ctx = _Ctx()
    off.GetZoneOccupancy(P.ZoneRequest(stream_id=0), ctx)
    assert ctx.code == grpc.StatusCode.FAILED_PRECONDITION and "--serve_zones" in ctx.details
    ctx = _Ctx()
    on.GetZoneOccupancy(P.ZoneRequest(stream_id=5), ctx)
    assert ctx.code == grpc.StatusCode.NOT_FOUND
    ctx = _Ctx()
    on.GetZoneOccupancy(P.ZoneRequest(stream_id=0), ctx)
    assert ctx.code == grpc.StatusCode.UNAVAILABLE
    hub.push_zones(_rows(2, 3, False, [1]), np.array([[1, 0, 0.5]]))
    ctx = _Ctx()
    m = on.GetZoneOccupancy(P.ZoneRequest(stream_id=0), ctx)
    assert ctx.code is None and len(m.zones) == 2 and m.zones[1].name == "a"


def _known_words(conf):
    """R = 3, C = 4, N = 100 (20 pixels hold a label past the classes)."""
    w = np.zeros(ZN.frame_words(3, 4, conf), np.uint32)
    w[:4] = (3, 100, 10, 10)
    px = np.array([[10, 50, 0, 20], [5, 5, 0, 7], [0, 0, 0, 0]], np.uint32)
    w[4:16] = px.reshape(-1)
    if conf:
        sc = np.array([[255 * 10, 128 * 50, 0, 20], [5, 1000, 0, 0], [0, 0, 0, 0]], np.uint32)
        w[16:] = sc.reshape(-1)
    return w


def test_float_fields_and_class_order_come_from_the_integers():
    hub = ResultHub(1)
    hub.put_zones(0, 4, 9.5, _known_words(True), conf=True)
    sv = S.SemanticSegmentationV2Servicer(hub, {0: "background", 1: "car", 3: "person"},
                                          zone_names=["frame", "door", "bay"], model_size=(16, 12))
    m = sv.GetZoneOccupancy(P.ZoneRequest(stream_id=0), _Ctx())
    assert (m.stream_id, m.frame_id, m.timestamp, m.width, m.height) == (0, 4, 9.5, 10, 10)
    assert (m.model_width, m.model_height, m.has_confidence) == (16, 12, True)
    f32 = np.float32
    fr, door, bay = m.zones
    assert [(z.index, z.name, z.pixels) for z in m.zones] == [(0, "frame", 80), (1, "door", 17), (2, "bay", 0)]
    assert fr.area == f32(80 / 100) and door.area == f32(17 / 100) and bay.area == 0.0 and len(bay.classes) == 0
    # pixels descending, then class_id ascending; classes without a pixel are left out
    assert [(c.class_id, c.label, c.pixels) for c in fr.classes] == [(1, "car", 50), (3, "person", 20), (0, "background", 10)]
    assert [(c.class_id, c.pixels) for c in door.classes] == [(3, 7), (0, 5), (1, 5)]
    assert [c.share for c in fr.classes] == [f32(50 / 80), f32(20 / 80), f32(10 / 80)]
    assert [c.confidence for c in fr.classes] == [f32(128 * 50 / (255 * 50)), f32(20 / (255 * 20)), f32(1.0)]
    assert [c.confidence for c in door.classes] == [0.0, f32(5 / (255 * 5)), f32(1000 / (255 * 5))]
    hub.put_zones(0, 5, 9.5, _known_words(False))
    m = sv.GetZoneOccupancy(P.ZoneRequest(stream_id=0), _Ctx())
    assert not m.has_confidence and all(c.confidence == 0.0 for z in m.zones for c in z.classes)
    assert [(c.class_id, c.pixels) for c in m.zones[1].classes] == [(3, 7), (0, 5), (1, 5)]


def test_loopback_rpc():
    hub = ResultHub(2)
    hub.put_zones(1, 42, 123.25, _known_words(True), conf=True)
    server = grpc.server(futures.ThreadPoolExecutor(max_workers=2))
    port = server.add_insecure_port("127.0.0.1:0")
    S.add_v2_servicer(S.SemanticSegmentationV2Servicer(hub, {}, zone_names=["frame", "door", "bay"],
                                                       model_size=(33, 33)), server)
    server.start()
    try:
        with grpc.insecure_channel(f"127.0.0.1:{port}") as ch:
            stub = S.SemanticSegmentationV2Stub(ch)
            m = stub.GetZoneOccupancy(P.ZoneRequest(stream_id=1))
            assert (m.stream_id, m.frame_id, m.timestamp) == (1, 42, 123.25)
            assert (m.width, m.height, m.model_width, m.model_height) == (10, 10, 33, 33)
            assert [z.name for z in m.zones] == ["frame", "door", "bay"] and m.has_confidence
            assert [(c.class_id, c.pixels) for c in m.zones[0].classes] == [(1, 50), (3, 20), (0, 10)]
            with pytest.raises(grpc.RpcError) as e:
                stub.GetZoneOccupancy(P.ZoneRequest(stream_id=0))
            assert e.value.code() == grpc.StatusCode.UNAVAILABLE
            with pytest.raises(grpc.RpcError) as e:
                stub.GetZoneOccupancy(P.ZoneRequest(stream_id=9))
            assert e.value.code() == grpc.StatusCode.NOT_FOUND
    finally:
        server.stop(0)


def test_v2_has_the_rpc_and_the_readable_proto_lists_it():
    import os
    assert "GetZoneOccupancy" in P.V2_METHODS and "GetZoneOccupancy" not in P.V1_METHODS
    v2 = {m.name: {f.name: (f.number, f.type) for f in m.field} for m in P.v2_file_descriptor().message_type}
    F = P.F
    assert v2["ZoneRequest"] == {"stream_id": (1, F.TYPE_INT32)}
    assert v2["ZoneClass"] == {"class_id": (1, F.TYPE_INT32), "label": (2, F.TYPE_STRING),
                               "pixels": (3, F.TYPE_UINT32), "share": (4, F.TYPE_FLOAT),
                               "confidence": (5, F.TYPE_FLOAT)}
    assert v2["Zone"] == {"index": (1, F.TYPE_INT32), "name": (2, F.TYPE_STRING), "pixels": (3, F.TYPE_UINT32),
                          "area": (4, F.TYPE_FLOAT), "classes": (5, F.TYPE_MESSAGE)}
    assert v2["ZoneOccupancy"] == {
        "stream_id": (1, F.TYPE_INT32), "frame_id": (2, F.TYPE_INT64), "timestamp": (3, F.TYPE_DOUBLE),
        "width": (4, F.TYPE_INT32), "height": (5, F.TYPE_INT32), "model_width": (6, F.TYPE_INT32),
        "model_height": (7, F.TYPE_INT32), "zones": (8, F.TYPE_MESSAGE), "has_confidence": (9, F.TYPE_BOOL)}
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                        "semantic_segmentation_server_amd", "api", "sem_seg_server_v2.proto")
    with open(path) as f:
        text = f.read()
    assert "rpc GetZoneOccupancy(ZoneRequest) returns (ZoneOccupancy)" in text
    for name, fields in v2.items():
        if name.startswith("Zone"):
            assert f"message {name} " in text
            for fname, (num, _) in fields.items():
                assert f" {fname} = {num};" in text, (name, fname)


# ---- serving on the CPU ------------------------------------------------------------------------

@pytest.mark.parametrize("serve", [True, False])
def test_server_and_client_on_cpu(serve, zone_file, capsys):
    from semantic_segmentation_server_amd import client
    from semantic_segmentation_server_amd.server import Server
    kw = dict(serve_zones=True, zones=zone_file, serve_confidence=True) if serve else {}
    srv = Server(_cfg(fps_limit=None, **kw), max_steps=3).start()
    try:
        srv.producer.join(timeout=120)
        assert srv.producer.steps == 3 and srv.producer.error is None
        target = f"127.0.0.1:{srv.port}"
        if not serve:
            with grpc.insecure_channel(target) as ch:
                with pytest.raises(grpc.RpcError) as e:
                    S.SemanticSegmentationV2Stub(ch).GetZoneOccupancy(P.ZoneRequest(stream_id=0))
            assert e.value.code() == grpc.StatusCode.FAILED_PRECONDITION
            assert client.main(["--target", target, "--zones_of"]) == 1
            return
        m = client.fetch_zones(target, 0)
        eng = srv.engine
        assert (m.width, m.height) == (eng.crop_w, eng.crop_h) and m.frame_id == 2 and m.has_confidence
        assert (m.model_width, m.model_height) == (65, 65)
        t = ZN.decode(srv.hub.zones(0).words, conf=True)
        assert [z.name for z in m.zones] == ["frame", "left", "right", "tri"]
        assert [z.pixels for z in m.zones] == t.pixels.sum(1).tolist()
        assert m.zones[0].pixels == eng.crop_w * eng.crop_h == m.zones[1].pixels + m.zones[2].pixels
        capsys.readouterr()
        assert client.main(["--target", target, "--zones_of", "0"]) == 0
        text = capsys.readouterr().out
        assert "frame 2" in text and "share" in text and "conf" in text and " px" in text
        for z in m.zones:
            assert z.name in text
        c = m.zones[0].classes[0]
        assert f"{c.label}" in text and f"{c.pixels} px" in text and f"share {c.share:.4f}" in text
        assert f"conf {c.confidence:.3f}" in text
    finally:
        srv.stop(0)


def test_supervised_server_on_cpu(zone_file):
    from semantic_segmentation_server_amd.runtime.supervisor import SupervisedServer
    sup = SupervisedServer(_cfg(serve_zones=True, zones=zone_file), heartbeat_timeout_s=60.0).start()
    try:
        t_end = time.time() + 240
        while sup.hub.zones(0) is None and time.time() < t_end and sup.alive:
            time.sleep(0.05)
        z = sup.hub.zones(0)
        assert z is not None, sup.error
        assert len(z.words) == 4 + 4 * 21 and int(z.words[0]) == 4 and int(z.words[2]) == 65 and not z.conf
        with grpc.insecure_channel(f"127.0.0.1:{sup.port}") as ch:
            m = S.SemanticSegmentationV2Stub(ch).GetZoneOccupancy(P.ZoneRequest(stream_id=0))
        assert m.frame_id >= z.frame_id and m.width == 65 and [x.name for x in m.zones][1:] == ["left", "right", "tri"]
        assert m.zones[0].pixels == m.width * m.height
    finally:
        sup.stop(0)


def test_multi_rank_group_is_rejected(zone_file):
    from semantic_segmentation_server_amd.parallel.dist import DistContext
    from semantic_segmentation_server_amd.parallel.dp import DataParallelPipeline
    from semantic_segmentation_server_amd.parallel.serving import serve_distributed
    from semantic_segmentation_server_amd.runtime.engine import Engine
    eng = Engine(_cfg(serve_zones=True, zones=zone_file))
    ctx = DistContext(rank=0, world=2, backend="gloo")  # an initialised world-2 gloo group
    with pytest.raises(ValueError, match="serve_zones"):
        DataParallelPipeline(ctx, eng, 160, 120, 1, "local", None)
    with pytest.raises(ValueError, match="serve_zones"):
        serve_distributed(_cfg(serve_zones=True, gpus=2, supervise=False))
    # world size 1 is fine, on the CPU too: the zones ride with the records
    hub = ResultHub(1)
    pipe = DataParallelPipeline(DistContext(), eng, 160, 120, 1, "local", hub, lag=1)
    f = torch.zeros((1, 120, 160, 3), dtype=torch.uint8)
    pipe.prefetch(f)
    pipe.step(frame_ids=[5], ts=[1.0], streams=[0])
    pipe.flush()
    z = hub.zones(0)
    assert z.frame_id == 5 and tuple(z.words[:4]) == (4, eng.crop_w * eng.crop_h, eng.crop_w, eng.crop_h)
