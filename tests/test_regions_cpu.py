"""Class regions (postprocess/regions.py): the numpy definition on maps whose regions are
written out by hand, its refusals, and the layers that carry the words on the CPU: hub,
supervisor channel, servicer, RPC, server.
"""
import json
import os
import threading
import time
from concurrent import futures

import grpc
import numpy as np
import pytest
import torch

from semantic_segmentation_server_amd import config as C
from semantic_segmentation_server_amd.api import proto as P
from semantic_segmentation_server_amd.api import service as S
from semantic_segmentation_server_amd.postprocess import regions as RG
from semantic_segmentation_server_amd.runtime.results import ResultHub


def _words(n_regions, cw, ch, recs, K):
    """The expected words, from hand-written (label, root, pixels, sum_x, sum_y, x_min, y_min,
    x_max, y_max) tuples."""
    w = np.zeros(4 + 6 * K, np.uint32)
    w[:4] = (n_regions, cw * ch, cw, ch)
    for i, (l, root, px, sx, sy, x0, y0, x1, y1) in enumerate(recs):
        w[4 + 6 * i:10 + 6 * i] = ((l << 24) | root, px, sx, sy, x0 | (y0 << 16), x1 | (y1 << 16))
    return w


def _map(rows):
    return np.array([[int(c) for c in r] for r in rows], np.uint8)


# ---- the definition -------------------------------------------------------------------------

def test_two_classes_touching():
    lab = _map(["1122",
                "1122",
                "0022"])
    got = RG.encode(lab, 4, 3, [1, 2], 1, 4)
    want = _words(2, 4, 3, [(2, 2, 6, 15, 6, 2, 0, 3, 2), (1, 0, 4, 2, 2, 0, 0, 1, 1)], 4)
    assert np.array_equal(got, want)
    # the crop cuts the map: the last column and row are not there
    got = RG.encode(lab, 3, 2, [1, 2], 1, 4)
    assert np.array_equal(got, _words(2, 3, 2, [(1, 0, 4, 2, 2, 0, 0, 1, 1), (2, 2, 2, 4, 1, 2, 0, 2, 1)], 4))


def test_a_diagonal_only_link_joins():
    lab = _map(["300",
                "030",
                "003"])
    got = RG.encode(lab, 3, 3, [3], 1, 2)
    assert np.array_equal(got, _words(1, 3, 3, [(3, 0, 3, 3, 3, 0, 0, 2, 2)], 2))
    lab = _map(["003",
                "030",
                "300"])
    got = RG.encode(lab, 3, 3, [3], 1, 2)
    assert np.array_equal(got, _words(1, 3, 3, [(3, 2, 3, 3, 3, 0, 0, 2, 2)], 2))


def test_an_excluded_class_separates_two_blobs_and_is_no_region():
    lab = _map(["11511",
                "11511"])
    got = RG.encode(lab, 5, 2, [1], 1, 4)
    want = _words(2, 5, 2, [(1, 0, 4, 2, 2, 0, 0, 1, 1), (1, 3, 4, 14, 2, 3, 0, 4, 1)], 4)
    assert np.array_equal(got, want)
    got = RG.encode(lab, 5, 2, [1, 5], 1, 4)  # served, the separator is a region of its own
    want = _words(3, 5, 2, [(1, 0, 4, 2, 2, 0, 0, 1, 1), (1, 3, 4, 14, 2, 3, 0, 4, 1),
                            (5, 2, 2, 4, 1, 2, 0, 2, 1)], 4)
    assert np.array_equal(got, want)
    assert RG.default_classes(21) == (1 << 21) - 2 and RG.class_mask([1, 5]) == 0b100010


def test_an_area_tie_is_ordered_by_root_and_min_pixels_drops():
    lab = _map(["2201",
                "0001",
                "3300"])
    got = RG.encode(lab, 4, 3, [1, 2, 3], 2, 4)
    want = _words(3, 4, 3, [(2, 0, 2, 1, 0, 0, 0, 1, 0), (1, 3, 2, 6, 1, 3, 0, 3, 1),
                            (3, 8, 2, 1, 4, 0, 2, 1, 2)], 4)
    assert np.array_equal(got, want)
    lab[2, 2] = 3  # now the largest
    got = RG.encode(lab, 4, 3, [1, 2, 3], 3, 4)
    assert np.array_equal(got, _words(1, 4, 3, [(3, 8, 3, 3, 6, 0, 2, 2, 2)], 4))


def test_more_than_k_regions_keeps_the_true_count_and_k_records():
    lab = _map(["10203",
                "00000",
                "40506"])
    out = np.full(4 + 6 * 2, 0xABCD, np.uint32)
    got = RG.encode(lab, 5, 3, range(1, 7), 1, 2, out=out)
    want = _words(6, 5, 3, [(1, 0, 1, 0, 0, 0, 0, 0, 0), (2, 2, 1, 2, 0, 2, 0, 2, 0)], 2)
    assert got is out and np.array_equal(got, want) and RG.used_words(got) == 16
    tab = RG.decode(got)
    assert len(tab) == 2 and tab["label"].tolist() == [1, 2] and tab["root"].tolist() == [0, 2]
    one = RG.encode(lab, 5, 3, [6], 1, 2, out=np.full(16, 0xABCD, np.uint32))
    assert RG.used_words(one) == 10 and (one[10:] == 0xABCD).all()  # words past the used ones: not written
    none = RG.encode(lab, 5, 3, [9], 1, 2)
    assert none[0] == 0 and RG.used_words(none) == 4 and len(RG.decode(none)) == 0


def test_numpy_labelling_equals_scipy_per_class():
    ndimage = pytest.importorskip("scipy.ndimage")
    from semantic_segmentation_server_amd.postprocess import synthetic
    rng = np.random.default_rng(0)
    for _ in range(50):
        h, w = int(rng.integers(20, 90)), int(rng.integers(20, 90))
        lab = synthetic.random_label_map(rng, h, w, block=16).astype(np.uint8)
        sp = rng.random((h, w)) < 0.05
        lab[sp] = rng.integers(0, 21, int(sp.sum()))
        served = [int(c) for c in np.unique(lab) if c != 0]
        mine = RG.label_components(lab, RG.class_mask(served))
        assert ((mine < 0) == (lab == 0)).all()
        for c in served:
            ref, n = ndimage.label(lab == c, structure=np.ones((3, 3)))
            flat = np.arange(h * w).reshape(h, w)
            for k in range(1, n + 1):
                sel = ref == k
                assert (mine[sel] == flat[sel].min()).all()
        tab = RG.region_table(lab, w, h, served, 1)
        assert int(tab["pixels"].sum()) == int((lab != 0).sum())


def test_check_geometry_refusals_name_the_flag():
    RG.check_geometry(513, 385, 527, 64)
    RG.check_geometry(64, 64, 1, 256)  # 4096 candidates exactly
    with pytest.raises(ValueError, match="input_size"):
        RG.check_geometry(4096, 4096, 100000, 64)           # N >= 2^24
    with pytest.raises(ValueError, match="input_size"):
        RG.check_geometry(2000, 2000, 4000, 64)             # N * max >= 2^32
    with pytest.raises(ValueError, match="max_regions"):
        RG.check_geometry(64, 64, 1, 0)
    with pytest.raises(ValueError, match="max_regions"):
        RG.check_geometry(64, 64, 1, 257)
    with pytest.raises(ValueError, match="region_min_area_ratio"):
        RG.check_geometry(64, 64, 0, 8)
    with pytest.raises(ValueError, match="region_min_area_ratio"):
        RG.check_geometry(65, 64, 1, 8)                     # 4160 > REGION_CANDIDATES
    with pytest.raises(ValueError):
        RG.check_geometry(0, 5, 1, 8)
    with pytest.raises(ValueError):
        RG.encode(np.zeros((4, 4), np.int32), 4, 4, [1], 1, 2)
    with pytest.raises(ValueError):
        RG.encode(np.zeros((4, 4), np.uint8), 5, 4, [1], 1, 2)
    with pytest.raises(ValueError):
        RG.class_mask([256])
    assert RG.min_pixels_for(0.002, 513, 513) == 527 and RG.min_pixels_for(0.0, 65, 65) == 1


def test_engine_refuses_a_bad_geometry_when_built():
    from semantic_segmentation_server_amd.runtime.engine import Engine
    with pytest.raises(ValueError, match="max_regions"):
        Engine(_cfg(serve_regions=True, max_regions=300))
    with pytest.raises(ValueError, match="region_min_area_ratio"):
        Engine(_cfg(serve_regions=True, region_min_area_ratio=0.0))  # 65 * 65 one-pixel regions
    with pytest.raises(ValueError, match="region_classes"):
        Engine(_cfg(serve_regions=True, region_classes="person,unicorn"))
    eng = Engine(_cfg(serve_regions=True, region_classes="person, 7"))
    assert eng.region_mask == (1 << 15) | (1 << 7) and eng.region_cap == 64
    assert eng.region_min_pixels == int(np.ceil(0.002 * 65 * 65))
    assert Engine(_cfg()).region_cap == 0


# ---- hub, channel -----------------------------------------------------------------------------

def _rows(maps, K, classes=range(1, 21), min_pixels=1):
    return np.stack([RG.encode(m, m.shape[1], m.shape[0], classes, min_pixels, K) for m in maps])


def _three_maps():
    a = _map(["1100", "1100", "0022"])
    b = _map(["3333", "0000", "4004"])
    c = _map(["5050", "0505", "5050"])
    return [a, b, c]


def test_hub_keeps_the_latest_regions_per_stream():
    maps = _three_maps()
    rows = _rows(maps, 4)
    hub = ResultHub(2)
    assert hub.regions(0) is None
    hub.push_regions(rows.view(np.int32), np.array([[10, 0, 1.0], [11, 1, 1.5], [12, 0, 2.0]]))
    r0, r1 = hub.regions(0), hub.regions(1)
    assert (r0.frame_id, r0.ts, r1.frame_id, r1.ts) == (12, 2.0, 11, 1.5)
    assert np.array_equal(r0.words, rows[2][:RG.used_words(rows[2])]) and len(r0.words) == 4 + 6
    assert np.array_equal(r1.words, rows[1][:RG.used_words(rows[1])]) and len(r1.words) == 4 + 18
    rows[2][:] = 0  # the hub holds copies
    assert hub.regions(0).words[0] == 1
    hub.push_regions(rows[:1], np.array([[13, 1, 3.0]]))
    assert hub.regions(1).frame_id == 13 and hub.regions(0).frame_id == 12
    assert hub.mask(0) is None  # masks and regions are kept apart


def test_region_channel_round_trip_and_no_torn_row():
    from semantic_segmentation_server_amd.runtime.supervisor import _RingHub, _WordChannel
    maps = _three_maps()
    rows = _rows(maps, 4)
    ch = _WordChannel(streams=2, cap=4, first=4, unit=6)
    try:
        peer = _WordChannel(name=ch.name)  # the worker's attachment
        assert (peer.S, peer.cap, peer.first, peer.unit) == (2, 4, 4, 6) and ch.pull() == []
        hub = _RingHub(None, None, peer)
        hub.push_regions(rows[:2], np.array([[7, 4, 1.0], [8, 4, 2.0]]))  # one stream: the last frame
        hub.push_regions(rows[2:], np.array([[3, 5, 0.5]]))
        hub.push_regions(rows[:1], np.array([[1, 9, 0.0]]))  # not this worker's stream: ignored
        got = ch.pull()
        assert [(s, f, t) for s, f, t, _ in got] == [(4, 8, 2.0), (5, 3, 0.5)]
        assert np.array_equal(got[0][3], rows[1][:RG.used_words(rows[1])])
        assert np.array_equal(got[1][3], rows[2][:RG.used_words(rows[2])])
        assert ch.pull() == []
        # a slot caught mid-write (odd sequence) is skipped: the reader keeps what it has
        k = peer._writes[0]
        peer.meta[2 * 0 + (k & 1)][0] = 2 * k + 1
        assert ch.pull() == []
        peer.write(4, 9, 3.0, rows[2][:RG.used_words(rows[2])])
        got = ch.pull()
        assert [(s, f) for s, f, _, _ in got] == [(4, 9)] and np.array_equal(got[0][3], rows[2][:10])
        # a writer that keeps rewriting while the parent reads: every row taken is one the
        # worker wrote, whole (row v holds v regions, every record word equal to v)
        def row(v):
            w = np.full(4 + 6 * v, v, np.uint32)
            w[:4] = (v, 12, 4, 3)
            return w
        stop = threading.Event()

        def writer():
            v = 0
            while not stop.is_set():
                v = v % 4 + 1
                peer.write(5, v, float(v), row(v))
        th = threading.Thread(target=writer)
        th.start()
        try:
            seen = 0
            for _ in range(3000):
                for s, f, t, w in ch.pull():
                    assert s == 5 and t == float(f) and np.array_equal(w, row(f))
                    seen += 1
        finally:
            stop.set()
            th.join()
        assert seen > 0
        peer.close()
    finally:
        ch.close()


# ---- servicer and RPC ---------------------------------------------------------------------------

class _Ctx:
    code = None

    def set_code(self, c):
        self.code = c

    def set_details(self, d):
        self.details = d


def test_status_codes():
    hub = ResultHub(1)
    on = S.SemanticSegmentationV2Servicer(hub, {}, serve_regions=True, model_size=(9, 9))
    off = S.SemanticSegmentationV2Servicer(hub, {}, serve_masks=True)
    ctx = _Ctx()
    off.GetClassRegions(P.RegionRequest(stream_id=0), ctx)
    assert ctx.code == grpc.StatusCode.FAILED_PRECONDITION and "--serve_regions" in ctx.details
    ctx = _Ctx()
    on.GetClassRegions(P.RegionRequest(stream_id=5), ctx)
    assert ctx.code == grpc.StatusCode.NOT_FOUND
    ctx = _Ctx()
    on.GetClassRegions(P.RegionRequest(stream_id=0), ctx)
    assert ctx.code == grpc.StatusCode.UNAVAILABLE
    hub.push_regions(_rows([np.full((3, 3), 2, np.uint8)], 8), np.array([[1, 0, 0.5]]))
    ctx = _Ctx()
    m = on.GetClassRegions(P.RegionRequest(stream_id=0), ctx)
    assert ctx.code is None and len(m.regions) == 1 and m.regions[0].pixels == 9


def test_float_fields_come_from_the_integer_words():
    lab = np.zeros((6, 8), np.uint8)
    lab[1:4, 2:7] = 15   # 15 pixels: x 2 .. 6, y 1 .. 3
    lab[5, 0:2] = 7      # 2 pixels
    lab[0, 7] = 3        # 1 pixel
    rows = _rows([lab], 2)  # K = 2: the third region is cut off
    assert rows[0, 0] == 3
    hub = ResultHub(1)
    hub.push_regions(rows, np.array([[4, 0, 9.5]]))
    sv = S.SemanticSegmentationV2Servicer(hub, {15: "person", 7: "car"}, serve_regions=True,
                                          model_size=(16, 8))
    m = sv.GetClassRegions(P.RegionRequest(stream_id=0), _Ctx())
    assert (m.stream_id, m.frame_id, m.timestamp, m.width, m.height) == (0, 4, 9.5, 8, 6)
    assert (m.model_width, m.model_height, m.total_regions, m.truncated) == (16, 8, 3, True)
    f32 = np.float32
    a, b = m.regions
    assert (a.label, a.class_id, a.pixels, b.label, b.class_id, b.pixels) == ("person", 15, 15, "car", 7, 2)
    assert a.area == f32(15 / 128) and b.area == f32(2 / 128)
    assert a.cx == f32((60 / 15 + 0.5) / 16) and a.cy == f32((30 / 15 + 0.5) / 8)
    assert b.cx == f32((1 / 2 + 0.5) / 16) and b.cy == f32((10 / 2 + 0.5) / 8)
    assert (a.x_min, a.y_min, a.x_max, a.y_max) == (f32(2 / 16), f32(1 / 8), f32(7 / 16), f32(4 / 8))
    assert (b.x_min, b.y_min, b.x_max, b.y_max) == (0.0, f32(5 / 8), f32(2 / 16), f32(6 / 8))
    one = sv.GetClassRegions(P.RegionRequest(stream_id=0, max_regions=1), _Ctx())
    assert len(one.regions) == 1 and one.regions[0] == a and one.truncated and one.total_regions == 3


def test_loopback_rpc():
    maps = _three_maps()
    hub = ResultHub(2)
    hub.push_regions(_rows(maps[1:2], 8), np.array([[42, 1, 123.25]]))
    server = grpc.server(futures.ThreadPoolExecutor(max_workers=2))
    port = server.add_insecure_port("127.0.0.1:0")
    S.add_v2_servicer(S.SemanticSegmentationV2Servicer(hub, {}, serve_regions=True, model_size=(33, 33)),
                      server)
    server.start()
    try:
        with grpc.insecure_channel(f"127.0.0.1:{port}") as ch:
            stub = S.SemanticSegmentationV2Stub(ch)
            m = stub.GetClassRegions(P.RegionRequest(stream_id=1))
            assert (m.stream_id, m.frame_id, m.timestamp) == (1, 42, 123.25)
            assert (m.width, m.height, m.model_width, m.model_height) == (4, 3, 33, 33)
            assert not m.truncated and m.total_regions == 3
            assert [(r.class_id, r.pixels) for r in m.regions] == [(3, 4), (4, 1), (4, 1)]
            with pytest.raises(grpc.RpcError) as e:
                stub.GetClassRegions(P.RegionRequest(stream_id=0))
            assert e.value.code() == grpc.StatusCode.UNAVAILABLE
            with pytest.raises(grpc.RpcError) as e:
                stub.GetClassRegions(P.RegionRequest(stream_id=9))
            assert e.value.code() == grpc.StatusCode.NOT_FOUND
    finally:
        server.stop(0)


def test_v2_has_the_rpc_and_v1_is_unchanged():
    assert "GetClassRegions" in P.V2_METHODS and "GetClassRegions" not in P.V1_METHODS
    names = [m.name for m in P.v1_file_descriptor().message_type]
    assert names == ["SegmentedObject", "SegmentedObjectData", "CameraResolution", "Empty"]
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                           "sem_seg_server_v1_descriptor.json")) as f:
        ref = json.load(f)
    ours = P.v1_file_descriptor()
    assert {tuple(m) for m in ref["methods"]} == \
        {(m.name, m.input_type, m.output_type) for s in ours.service for m in s.method}
    top = {m.name: sorted((f.name, f.number, f.type, f.label, f.type_name) for f in m.field)
           for m in ours.message_type}
    for name, fields in top.items():
        assert [tuple(f) for f in ref["messages"][name]] == fields
    v2 = P.v2_file_descriptor()
    assert {"RegionRequest", "ClassRegion", "ClassRegions"} <= {m.name for m in v2.message_type}


def test_the_readable_v2_proto_lists_every_v2_method_and_message():
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                        "semantic_segmentation_server_amd", "api", "sem_seg_server_v2.proto")
    with open(path) as f:
        text = f.read()
    v2 = P.v2_file_descriptor()
    for m in v2.message_type:
        assert f"message {m.name} " in text, m.name
        for fld in m.field:
            assert f" {fld.name} = {fld.number};" in text, (m.name, fld.name)
    for m in v2.service[0].method:
        assert f"rpc {m.name}(" in text, m.name


# ---- serving on the CPU -------------------------------------------------------------------------

def _cfg(**kw):
    base = dict(backend="torch", device="cpu", input_size=65, batch=1, port=0, host="127.0.0.1",
                min_area_ratio=0.0005, fps_limit=200.0, log_level="WARNING")
    base.update(kw)
    return C.Config(**base)


def test_cli_flags():
    cfg = C.parse(["--serve_regions", "--max_regions", "8", "--region_min_area_ratio", "0.01",
                   "--region_classes", "person,car"])
    assert (cfg.serve_regions, cfg.max_regions, cfg.region_min_area_ratio, cfg.region_classes) == \
        (True, 8, 0.01, "person,car")
    d = C.parse([])
    assert (d.serve_regions, d.max_regions, d.region_min_area_ratio, d.region_classes) == \
        (False, 64, 0.002, None)


def test_engine_step_regions_on_cpu():
    from semantic_segmentation_server_amd.runtime.engine import Engine
    from semantic_segmentation_server_amd.runtime.sources import SyntheticSource
    eng = Engine(_cfg(serve_regions=True, batch=2))
    f, _, _ = SyntheticSource(160, 120, pool=2, seed=3).read_batch(2)
    recs = eng.step(f, [0, 1], [0.0, 0.0], [0, 1])
    with torch.no_grad():
        lab = eng._infer_eager(torch.from_numpy(f)).numpy()
    assert eng.regions.shape == (2, 4 + 6 * 64) and eng.regions.dtype == np.uint32
    for b in range(2):
        want = RG.encode(lab[b], eng.crop_w, eng.crop_h, RG.default_classes(21), eng.region_min_pixels, 64)
        assert np.array_equal(eng.regions[b], want)
    off = Engine(_cfg(batch=2))
    recs_off = off.step(f, [0, 1], [0.0, 0.0], [0, 1])
    assert off.regions is None and off.region_cap == 0 and recs.tobytes() == recs_off.tobytes()


@pytest.mark.parametrize("serve", [True, False])
def test_server_on_cpu(serve):
    from semantic_segmentation_server_amd.server import Server
    srv = Server(_cfg(serve_regions=serve, fps_limit=None, region_min_area_ratio=0.001), max_steps=3).start()
    try:
        srv.producer.join(timeout=120)
        assert srv.producer.steps == 3 and srv.producer.error is None
        with grpc.insecure_channel(f"127.0.0.1:{srv.port}") as ch:
            stub = S.SemanticSegmentationV2Stub(ch)
            if not serve:
                with pytest.raises(grpc.RpcError) as e:
                    stub.GetClassRegions(P.RegionRequest(stream_id=0))
                assert e.value.code() == grpc.StatusCode.FAILED_PRECONDITION
                return
            m = stub.GetClassRegions(P.RegionRequest(stream_id=0))
        eng = srv.engine
        assert (m.width, m.height) == (eng.crop_w, eng.crop_h) and m.frame_id == 2
        assert (m.model_width, m.model_height) == (65, 65)
        tab = RG.decode(srv.hub.regions(0).words)
        assert m.total_regions == int(srv.hub.regions(0).words[0]) and len(m.regions) == len(tab)
        assert [(r.class_id, r.pixels) for r in m.regions] == list(zip(tab["label"].tolist(), tab["pixels"].tolist()))
    finally:
        srv.stop(0)


def test_supervised_server_on_cpu():
    from semantic_segmentation_server_amd.runtime.supervisor import SupervisedServer
    sup = SupervisedServer(_cfg(serve_regions=True, region_min_area_ratio=0.001),
                           heartbeat_timeout_s=60.0).start()
    try:
        t_end = time.time() + 240
        while sup.hub.regions(0) is None and time.time() < t_end and sup.alive:
            time.sleep(0.05)
        r = sup.hub.regions(0)
        assert r is not None, sup.error
        assert len(r.words) == RG.used_words(r.words, 64) and int(r.words[2]) == 65
        with grpc.insecure_channel(f"127.0.0.1:{sup.port}") as ch:
            m = S.SemanticSegmentationV2Stub(ch).GetClassRegions(P.RegionRequest(stream_id=0))
        assert m.frame_id >= r.frame_id and m.width == 65
    finally:
        sup.stop(0)


def test_multi_rank_group_is_rejected():
    from semantic_segmentation_server_amd.parallel.dist import DistContext
    from semantic_segmentation_server_amd.parallel.dp import DataParallelPipeline
    from semantic_segmentation_server_amd.parallel.serving import serve_distributed
    from semantic_segmentation_server_amd.runtime.engine import Engine
    eng = Engine(_cfg(serve_regions=True))
    ctx = DistContext(rank=0, world=2, backend="gloo")  # an initialised world-2 gloo group
    with pytest.raises(ValueError, match="serve_regions"):
        DataParallelPipeline(ctx, eng, 160, 120, 1, "local", None)
    with pytest.raises(ValueError, match="serve_regions"):
        serve_distributed(_cfg(serve_regions=True, gpus=2, supervise=False))
    # world size 1 is fine, on the CPU too: the regions ride with the records
    hub = ResultHub(1)
    pipe = DataParallelPipeline(DistContext(), eng, 160, 120, 1, "local", hub, lag=1)
    f = torch.zeros((1, 120, 160, 3), dtype=torch.uint8)
    pipe.prefetch(f)
    pipe.step(frame_ids=[5], ts=[1.0], streams=[0])
    pipe.flush()
    r = hub.regions(0)
    assert r.frame_id == 5 and tuple(r.words[1:4]) == (eng.crop_w * eng.crop_h, eng.crop_w, eng.crop_h)
