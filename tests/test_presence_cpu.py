"""Zone presence (postprocess/presence.py) without a GPU: the definition on hand cases, its
invariants on the drifting-rectangle sequences, the limits, and the layers that carry the words
on the CPU: config, engine, hub, supervisor channel, servicer, RPC, server, client.
"""
import json
import time
from concurrent import futures

import grpc
import numpy as np
import pytest
import torch

import presence_cases as PC
from semantic_segmentation_server_amd import config as C
from semantic_segmentation_server_amd.api import proto as P
from semantic_segmentation_server_amd.api import service as S
from semantic_segmentation_server_amd.postprocess import presence as PR
from semantic_segmentation_server_amd.postprocess import regions as RG
from semantic_segmentation_server_amd.postprocess import tracks as TK
from semantic_segmentation_server_amd.runtime.results import ResultHub


# ---- the definition ------------------------------------------------------------------------------

def _hand():
    """A 4 x 6 crop: region A (class 1, 8 px, columns 0-1), region B (class 2, 4 px, columns 4-5 of
    the two top rows), one pixel of class 2 below min_pixels; zone 1 = columns 0-2, zone 2 =
    columns 1-4."""
    lab = np.zeros((4, 6), np.uint8)
    lab[:, 0:2] = 1
    lab[0:2, 4:6] = 2
    lab[3, 5] = 2
    plane = np.zeros((4, 6), np.uint32)
    plane[:, 0:3] |= 1
    plane[:, 1:5] |= 2
    return lab, plane


def test_hand_case_counts_and_words():
    lab, plane = _hand()
    w = PR.encode(lab, plane, 6, 4, [1, 2], 2, 4, 3, 512)
    assert w.dtype == np.uint32 and w.shape == (4 + 5 * 4,) == (PR.frame_words(4, 3),)
    assert w[:4].tolist() == [2, 24, 6, 4]
    p = PR.decode(w, 3)
    assert p.n == 2 and p.label.tolist() == [1, 2] and p.root.tolist() == [0, 4] and p.track_id.tolist() == [0, 0]
    assert p.P.tolist() == [[8, 8, 4], [4, 0, 2]] and p.D is None
    assert not w[4 + 5 * 2:].any()                      # zeros past entry n
    assert PR.inside(p.P, 512).tolist() == [[True, True, True], [True, False, True]]
    assert PR.inside(p.P, 513).tolist() == [[True, True, False], [True, False, False]]  # one step past a half
    assert PR.inside(p.P, 1).tolist() == [[True, True, True], [True, False, True]]      # P == 0 is never inside
    # K = 1: region B is past K and counts nowhere; row 0 alone without a plane
    w1 = PR.encode(lab, plane, 6, 4, [1, 2], 2, 1, 3, 512)
    assert w1.tolist() == [1, 24, 6, 4, (1 << 24) | 0, 0, 8, 8, 4]
    w0 = PR.encode(lab, None, 6, 4, [1, 2], 2, 4, 1, 512)
    assert w0[:4].tolist() == [2, 24, 6, 4] and PR.decode(w0, 1).P.tolist() == [[8], [4]]
    with pytest.raises(ValueError, match="zone plane"):
        PR.encode(lab, None, 6, 4, [1, 2], 2, 4, 3, 512)
    out = np.full(PR.frame_words(4, 3), 7, np.uint32)
    assert PR.encode(lab, plane, 6, 4, [1, 2], 2, 4, 3, 512, out=out) is out and np.array_equal(out, w)


def test_quantize_and_unit():
    assert PR.quantize(0.5) == 512 and PR.quantize(1.0) == 1024 and PR.quantize(1e-9) == 1
    assert PR.quantize(PR.DEFAULT_MIN_SHARE) == 512
    for bad in (0.0, -0.1, 1.0001):
        with pytest.raises(ValueError, match="--presence_min_share"):
            PR.quantize(bad)
    assert PR.unit(33) == 35 and PR.unit(33, True) == 68 and PR.unit(1) == 3
    assert PR.frame_words(256, 33, True) == 4 + 68 * 256


def test_hand_case_dwell():
    """One region of 4 px that moves across zone 1 (columns 0-1 of a 1 x 8 crop)."""
    plane = np.zeros((1, 8), np.uint32)
    plane[0, 0:2] = 1
    tr, dw = TK.StreamTracker(256), PR.StreamDwell()
    got = []
    for x0 in (0, 0, 1, 2, 1, 0):
        lab = np.zeros((1, 8), np.uint8)
        lab[0, x0:x0 + 4] = 1
        reg = RG.encode(lab, 8, 1, [1], 1, 2, tracker=tr)
        w = PR.encode(lab, plane, 8, 1, [1], 1, 2, 2, 512, tab=RG.decode(reg, tracks=True), dwell=dw)
        p = PR.decode(w, 2, tracks=True)
        got.append((int(p.track_id[0]), p.P[0].tolist(), p.D[0].tolist()))
    # 2 of 4 px: inside at q = 512; 1 of 4: outside, the dwell drops to 0; back in: restarts at 1
    assert got == [(1, [4, 2], [1, 1]), (1, [4, 2], [2, 2]), (1, [4, 1], [3, 0]), (1, [4, 0], [4, 0]),
                   (1, [4, 1], [5, 0]), (1, [4, 2], [6, 1])]
    dw.reset()
    tr.reset()
    lab = np.zeros((1, 8), np.uint8)
    lab[0, 0:4] = 1
    reg = RG.encode(lab, 8, 1, [1], 1, 2, tracker=tr)
    w = PR.encode(lab, plane, 8, 1, [1], 1, 2, 2, 512, tab=RG.decode(reg, tracks=True), dwell=dw)
    assert PR.decode(w, 2, tracks=True).D[0].tolist() == [1, 1]
    with pytest.raises(ValueError, match="stored regions"):
        PR.encode(lab, plane, 8, 1, [1], 1, 2, 2, 512, tab=np.zeros(0, RG.REGION_DTYPE), dwell=dw)


def test_encode_decode_round_trip():
    rng = np.random.default_rng(5)
    for tracks in (False, True):
        K, R = 5, 4
        w = np.zeros(PR.frame_words(K, R, tracks), np.uint32)
        n = 3
        w[:4] = (n, 70, 10, 7)
        body = rng.integers(0, 1 << 32, (n, PR.unit(R, tracks)), dtype=np.uint64).astype(np.uint32)
        w[4:4 + body.size] = body.reshape(-1)
        p = PR.decode(w.view(np.int32), R, tracks)
        assert (p.n, p.pixels_total, p.crop_w, p.crop_h) == (3, 70, 10, 7)
        assert np.array_equal(p.label, (body[:, 0] >> 24).astype(np.uint8))
        assert np.array_equal(p.root, body[:, 0] & 0xFFFFFF) and np.array_equal(p.track_id, body[:, 1])
        assert np.array_equal(p.P, body[:, 2:2 + R])
        assert (p.D is None) if not tracks else np.array_equal(p.D, body[:, 2 + R:])
        assert PR.used_words(w, R, tracks) == 4 + 3 * PR.unit(R, tracks)
        assert PR.decode(w[:PR.used_words(w, R, tracks)], R, tracks).n == 3  # the used words suffice
        with pytest.raises(ValueError, match="presence.decode"):
            PR.decode(w[:PR.used_words(w, R, tracks) - 1], R, tracks)
    with pytest.raises(ValueError, match="presence.decode"):
        PR.decode(np.array([1, 70, 10, 8, 0, 0, 0], np.uint32), 1)  # N != crop_w * crop_h


def test_the_sequences_contain_what_the_dwell_tests_need():
    o0, o1 = PC.sequence_oracles()
    q = PC.PRESENCE_Q
    hist = {}  # (stream, track id) -> [(age, P, D)] in frame order
    split = exact = below = False
    for s, rows in enumerate((o0, o1)):
        prev_ids = set()
        for reg, w in rows:
            tab, p = RG.decode(reg, tracks=True), PR.decode(w, 4, tracks=True)
            # the invariants of every frame
            assert p.n == len(tab) and np.array_equal(p.P[:, 0], tab["pixels"])
            assert np.array_equal(p.D[:, 0], tab["age"]) and np.array_equal(p.track_id, tab["track_id"])
            assert np.array_equal(p.P[:, 1] + p.P[:, 2], p.P[:, 0])   # left | right partition the crop
            ins = PR.inside(p.P, q)
            assert ((p.D > 0) == ins).all()
            for a in range(p.n):
                hist.setdefault((s, int(p.track_id[a])), []).append((int(tab["age"][a]), p.P[a].tolist(),
                                                                     p.D[a].tolist()))
                exact |= any(1024 * int(p.P[a, r]) == q * int(p.P[a, 0]) for r in (1, 2, 3))
                below |= any(1024 * (int(p.P[a, r]) + 1) >= q * int(p.P[a, 0]) > 1024 * int(p.P[a, r]) > 0
                             for r in (1, 2, 3))
            fresh = [a for a in range(p.n) if tab["age"][a] == 1 and tab["label"][a] == 1]
            split |= bool(prev_ids) and bool(fresh) and any(t in prev_ids for t in p.track_id.tolist())
            prev_ids = set(p.track_id.tolist())
    assert exact and below and split
    h = hist[(0, 1)]  # the block of stream 0
    assert [a for a, _, _ in h] == list(range(1, 9))                   # one track over all eight frames
    left = [d[1] for _, _, d in h]
    assert left == [1, 2, 3, 4, 5, 0, 1, 0]     # dwell >= 3, a leave while the age goes on, a re-entry
    assert h[4][1] == [100, 50, 50, h[4][1][3]] and h[5][1][:3] == [100, 49, 51]
    assert h[4][2][2] == 1 and h[5][2][2] == 2 and h[7][2][2] == 4     # right: the larger piece inherits
    assert h[7][1][0] == 60 and any(k[0] == 0 and v[0][1][0] == 30 for k, v in hist.items())  # the other piece is new
    assert max(d[3] for v in hist.values() for _, _, d in v) >= 2      # a dwell in the triangle too


def test_check_geometry_at_each_limit_and_one_past():
    PR.check_geometry(4096, 4095, 32, 256)          # N = 2^24 - 4096, Z = 32, K = 256
    PR.check_geometry(1, (1 << 24) - 1, 0, 1)       # N = 2^24 - 1
    for bad in ((4096, 4096, 0, 1), (513, 513, 33, 8), (513, 513, -1, 8), (513, 513, 4, 257),
                (513, 513, 4, 0), (0, 5, 0, 8), (5, 0, 0, 8)):
        with pytest.raises(ValueError, match="--serve_presence"):
            PR.check_geometry(*bad)
    assert PR.MAX_ZONES == 32 and PR.MAX_REGIONS == 256 and PR.NONE == 0xFFFF


# ---- config --------------------------------------------------------------------------------------

def test_cli_flags_and_every_refusal():
    d = C.parse([])
    assert (d.serve_presence, d.presence_min_share) == (False, 0.5)
    cfg = C.parse(["--serve_regions", "--serve_zones", "--serve_presence", "--presence_min_share", "0.25"])
    assert cfg.serve_presence and cfg.presence_min_share == 0.25 and not cfg.track_regions
    assert C.parse(["--serve_regions", "--serve_zones", "--serve_presence", "--track_regions"]).track_regions
    for argv in (["--serve_presence"], ["--serve_presence", "--serve_regions"],
                 ["--serve_presence", "--serve_zones"]):
        with pytest.raises(ValueError) as e:
            C.parse(argv)
        assert "--serve_presence" in str(e.value) and "--serve_regions" in str(e.value) \
            and "--serve_zones" in str(e.value)
    for share in ("0", "1.5", "-1"):
        with pytest.raises(ValueError, match="--presence_min_share"):
            C.parse(["--serve_regions", "--serve_zones", "--serve_presence", "--presence_min_share", share])
    with pytest.raises(ValueError, match="--track_regions"):   # dwell inherits that flag's refusals
        C.parse(["--serve_zones", "--serve_presence", "--track_regions"])


# ---- engine on the CPU ---------------------------------------------------------------------------

@pytest.fixture(scope="module")
def zone_file(tmp_path_factory):
    p = tmp_path_factory.mktemp("presence") / "zones.json"
    p.write_text(json.dumps(PC.ZONES))
    return str(p)


def _cfg(**kw):
    base = dict(backend="torch", device="cpu", input_size=65, batch=1, port=0, host="127.0.0.1",
                min_area_ratio=0.0005, fps_limit=200.0, log_level="WARNING")
    base.update(kw)
    return C.Config(**base)


def _on(zone_file, **kw):
    return _cfg(serve_regions=True, serve_zones=True, zones=zone_file, serve_presence=True, **kw)


@pytest.mark.parametrize("tracks", [False, True])
def test_engine_step_presence_on_cpu(tracks, zone_file):
    from semantic_segmentation_server_amd.runtime.engine import Engine
    from semantic_segmentation_server_amd.runtime.sources import SyntheticSource
    eng = Engine(_on(zone_file, track_regions=tracks, batch=2, streams=2, max_regions=8))
    src = SyntheticSource(160, 120, pool=4, seed=3)
    dw = [PR.StreamDwell(), PR.StreamDwell()]
    U = PR.unit(4, tracks)
    assert (eng.presence_rows, eng.presence_unit, eng.presence_q, eng.presence_tracks) == (4, U, 512, tracks)
    for step in range(3):
        f, _, _ = src.read_batch(2)
        recs = eng.step(f, [step, step], [0.0, 0.0], [0, 1])
        with torch.no_grad():
            lab, _ = eng._infer(torch.from_numpy(f))
        assert eng.presence.shape == (2, 4 + U * 8) and eng.presence.dtype == np.uint32
        for b in range(2):
            tab = RG.decode(eng.regions[b], tracks=True) if tracks else None
            want = PR.encode(lab[b].numpy(), eng.zone_plane, eng.crop_w, eng.crop_h, eng.region_mask,
                             eng.region_min_pixels, 8, 4, 512, tab=tab, dwell=dw[b] if tracks else None)
            assert np.array_equal(eng.presence[b], want)
            p = PR.decode(eng.presence[b], 4, tracks)
            rt = RG.decode(eng.regions[b], tracks=tracks)
            assert np.array_equal(p.P[:, 0], rt["pixels"]) and np.array_equal(p.P[:, 1] + p.P[:, 2], p.P[:, 0])
            if tracks:
                assert np.array_equal(p.D[:, 0], rt["age"]) and (step == 0 or p.n == 0 or p.D[:, 0].max() >= 1)
    off = Engine(_cfg(serve_regions=True, serve_zones=True, zones=zone_file, track_regions=tracks, batch=2,
                      streams=2, max_regions=8))
    f, _, _ = SyntheticSource(160, 120, pool=4, seed=3).read_batch(2)
    on2 = Engine(_on(zone_file, track_regions=tracks, batch=2, streams=2, max_regions=8))
    r_on, r_off = on2.step(f, [0, 0], [0.0, 0.0], [0, 1]), off.step(f, [0, 0], [0.0, 0.0], [0, 1])
    assert off.presence is None and off.presence_rows == 0 and r_on.tobytes() == r_off.tobytes()
    assert np.array_equal(on2.regions, off.regions) and np.array_equal(on2.zones, off.zones)
    if tracks:  # reset_tracks clears the dwell with the tracks
        eng.reset_tracks()
        f, _, _ = src.read_batch(2)
        eng.step(f, [9, 9], [0.0, 0.0], [0, 1])
        p = PR.decode(eng.presence[0], 4, True)
        assert p.n == 0 or int(p.D.max()) == 1


def test_engine_refuses_the_flag_without_its_two_parents(zone_file):
    from semantic_segmentation_server_amd.runtime.engine import Engine
    cfg = _on(zone_file)
    for name in ("serve_regions", "serve_zones"):
        bad = cfg.replace()
        object.__setattr__(bad, name, False)
        if name == "serve_zones":
            object.__setattr__(bad, "zones", None)
        with pytest.raises(ValueError, match="--serve_presence"):
            Engine(bad)


# ---- hub, channel, servicer ----------------------------------------------------------------------

def _row(K, R, tracks, entries, crop=(10, 10)):
    """One frame's words from [(label, root, track_id, P[R], D[R] or None)]."""
    U = PR.unit(R, tracks)
    w = np.zeros(PR.frame_words(K, R, tracks), np.uint32)
    w[:4] = (len(entries), crop[0] * crop[1], crop[0], crop[1])
    for a, (lab, root, tid, Pr, Dr) in enumerate(entries):
        e = w[4 + U * a:4 + U * (a + 1)]
        e[0], e[1], e[2:2 + R] = (lab << 24) | root, tid if tracks else 0, Pr
        if tracks:
            e[2 + R:] = Dr
    return w


def test_hub_keeps_the_latest_per_stream():
    hub = ResultHub(2)
    assert hub.presence(0) is None
    rows = np.stack([_row(4, 2, False, [(1, 5, 0, [9, 3], None)] * n) for n in (1, 2, 3)])
    hub.push_presence(rows.view(np.int32), np.array([[10, 0, 1.0], [11, 1, 2.0], [12, 0, 3.0]]), PR.unit(2))
    p0, p1 = hub.presence(0), hub.presence(1)
    assert (p0.frame_id, p0.ts, p0.tracks) == (12, 3.0, False) and np.array_equal(p0.words, rows[2, :4 + 4 * 3])
    assert (p1.frame_id, p1.ts) == (11, 2.0) and len(p1.words) == 4 + 4 * 2   # only the used words
    rows[2] = 0
    assert hub.presence(0).words[0] == 3  # the hub's own copy
    hub.push_presence(_row(4, 2, True, [(1, 5, 7, [9, 3], [2, 1])])[None], np.array([[13, 0, 4.0]]),
                      PR.unit(2, True), tracks=True)
    p0 = hub.presence(0)
    assert p0.frame_id == 13 and p0.tracks and len(p0.words) == 4 + 6 and hub.presence(1).frame_id == 11


def test_word_channel_carries_whole_frames():
    from semantic_segmentation_server_amd.runtime.supervisor import _RingHub, _WordChannel
    U = PR.unit(3, True)
    ch = _WordChannel(2, 4, first=4, unit=U)
    try:
        rows = np.stack([_row(4, 3, True, [(1, 5, 7, [9, 3, 0], [2, 1, 0])] * n) for n in (4, 1)])
        _RingHub(None, presence=ch).push_presence(rows, np.array([[20, 4, 1.5], [21, 5, 2.5]]), U, tracks=True)
        got = {s: (fid, ts, w) for s, fid, ts, w in ch.pull()}
        assert set(got) == {4, 5} and got[4][:2] == (20, 1.5) and got[5][:2] == (21, 2.5)
        assert np.array_equal(got[4][2], rows[0]) and np.array_equal(got[5][2], rows[1, :4 + U])
        assert ch.pull() == []
        _RingHub(None).push_presence(rows, np.array([[20, 4, 1.5], [21, 5, 2.5]]), U)  # no channel: dropped
    finally:
        ch.close()


class _Ctx:
    code = None

    def set_code(self, c):
        self.code = c

    def set_details(self, d):
        self.details = d


def _servicer(hub, **kw):
    base = dict(zone_names=["frame", "door", "bay"], presence_q=512, model_size=(16, 12))
    base.update(kw)
    return S.SemanticSegmentationV2Servicer(hub, {1: "car", 3: "person"}, **base)


def test_status_codes():
    hub = ResultHub(1)
    on, off = _servicer(hub), _servicer(hub, presence_q=0)
    ctx = _Ctx()
    off.GetZonePresence(P.PresenceRequest(stream_id=0), ctx)
    assert ctx.code == grpc.StatusCode.FAILED_PRECONDITION and "--serve_presence" in ctx.details
    ctx = _Ctx()
    on.GetZonePresence(P.PresenceRequest(stream_id=5), ctx)
    assert ctx.code == grpc.StatusCode.NOT_FOUND
    ctx = _Ctx()
    on.GetZonePresence(P.PresenceRequest(stream_id=0), ctx)
    assert ctx.code == grpc.StatusCode.UNAVAILABLE
    hub.put_presence(0, 1, 0.5, _row(4, 3, False, [(1, 5, 0, [9, 3, 0], None)]))
    ctx = _Ctx()
    m = on.GetZonePresence(P.PresenceRequest(stream_id=0), ctx)
    assert ctx.code is None and len(m.regions) == 1 and m.regions[0].zones[0].name == "door"


def _known(tracks):
    return _row(4, 3, tracks, [(3, 17, 4, [100, 50, 49], [6, 2, 0]), (1, 2, 9, [30, 0, 30], [1, 0, 1]),
                               (1, 60, 10, [7, 0, 0], [3, 0, 0])])


def test_floats_and_inside_come_from_the_integers():
    hub = ResultHub(1)
    hub.put_presence(0, 4, 9.5, _known(True), tracks=True)
    m = _servicer(hub).GetZonePresence(P.PresenceRequest(stream_id=0), _Ctx())
    assert (m.stream_id, m.frame_id, m.timestamp, m.width, m.height) == (0, 4, 9.5, 10, 10)
    assert (m.model_width, m.model_height, m.has_tracks, m.min_share) == (16, 12, True, 0.5)
    f32 = np.float32
    a, b, c = m.regions
    assert [(r.index, r.label, r.class_id, r.root, r.pixels, r.track_id, r.age) for r in m.regions] == \
        [(0, "person", 3, 17, 100, 4, 6), (1, "car", 1, 2, 30, 9, 1), (2, "car", 1, 60, 7, 10, 3)]
    assert [(h.index, h.name, h.pixels, h.share, h.inside, h.dwell) for h in a.zones] == \
        [(1, "door", 50, f32(0.5), True, 2), (2, "bay", 49, f32(0.49), False, 0)]   # exactly half is inside
    assert [(h.index, h.name, h.pixels, h.share, h.inside, h.dwell) for h in b.zones] == [(2, "bay", 30, 1.0, True, 1)]
    assert len(c.zones) == 0                       # zones without a pixel are left out
    # the same integers at another q: 49 of 100 is inside from q = 501
    m = _servicer(hub, presence_q=501).GetZonePresence(P.PresenceRequest(stream_id=0), _Ctx())
    assert [h.inside for h in m.regions[0].zones] == [True, True] and m.min_share == f32(501 / 1024)
    hub.put_presence(0, 5, 9.5, _known(False)[:4 + 5 * 3])
    m = _servicer(hub).GetZonePresence(P.PresenceRequest(stream_id=0), _Ctx())
    assert not m.has_tracks and all(r.track_id == 0 and r.age == 0 for r in m.regions)
    assert [(h.pixels, h.inside, h.dwell) for h in m.regions[0].zones] == [(50, True, 0), (49, False, 0)]


def test_loopback_rpc():
    hub = ResultHub(2)
    hub.put_presence(1, 42, 123.25, _known(True), tracks=True)
    server = grpc.server(futures.ThreadPoolExecutor(max_workers=2))
    port = server.add_insecure_port("127.0.0.1:0")
    S.add_v2_servicer(_servicer(hub, model_size=(33, 33)), server)
    server.start()
    try:
        with grpc.insecure_channel(f"127.0.0.1:{port}") as ch:
            stub = S.SemanticSegmentationV2Stub(ch)
            m = stub.GetZonePresence(P.PresenceRequest(stream_id=1))
            assert (m.stream_id, m.frame_id, m.timestamp) == (1, 42, 123.25)
            assert (m.width, m.height, m.model_width, m.model_height) == (10, 10, 33, 33)
            assert [r.pixels for r in m.regions] == [100, 30, 7] and m.has_tracks
            assert [(h.name, h.dwell) for h in m.regions[0].zones] == [("door", 2), ("bay", 0)]
            with pytest.raises(grpc.RpcError) as e:
                stub.GetZonePresence(P.PresenceRequest(stream_id=0))
            assert e.value.code() == grpc.StatusCode.UNAVAILABLE
            with pytest.raises(grpc.RpcError) as e:
                stub.GetZonePresence(P.PresenceRequest(stream_id=9))
            assert e.value.code() == grpc.StatusCode.NOT_FOUND
    finally:
        server.stop(0)


def test_v2_has_the_rpc_and_the_readable_proto_lists_it():
    import os
    assert "GetZonePresence" in P.V2_METHODS and "GetZonePresence" not in P.V1_METHODS
    v2 = {m.name: {f.name: (f.number, f.type) for f in m.field} for m in P.v2_file_descriptor().message_type}
    F = P.F
    assert v2["PresenceRequest"] == {"stream_id": (1, F.TYPE_INT32)}
    assert v2["ZoneHit"] == {"index": (1, F.TYPE_INT32), "name": (2, F.TYPE_STRING), "pixels": (3, F.TYPE_UINT32),
                             "share": (4, F.TYPE_FLOAT), "inside": (5, F.TYPE_BOOL), "dwell": (6, F.TYPE_UINT32)}
    assert v2["RegionPresence"] == {
        "index": (1, F.TYPE_INT32), "label": (2, F.TYPE_STRING), "class_id": (3, F.TYPE_INT32),
        "root": (4, F.TYPE_UINT32), "pixels": (5, F.TYPE_UINT32), "track_id": (6, F.TYPE_UINT32),
        "age": (7, F.TYPE_UINT32), "zones": (8, F.TYPE_MESSAGE)}
    assert v2["ZonePresence"] == {
        "stream_id": (1, F.TYPE_INT32), "frame_id": (2, F.TYPE_INT64), "timestamp": (3, F.TYPE_DOUBLE),
        "width": (4, F.TYPE_INT32), "height": (5, F.TYPE_INT32), "model_width": (6, F.TYPE_INT32),
        "model_height": (7, F.TYPE_INT32), "regions": (8, F.TYPE_MESSAGE), "has_tracks": (9, F.TYPE_BOOL),
        "min_share": (10, F.TYPE_FLOAT)}
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                        "semantic_segmentation_server_amd", "api", "sem_seg_server_v2.proto")
    with open(path) as f:
        text = f.read()
    assert "rpc GetZonePresence(PresenceRequest) returns (ZonePresence)" in text
    for name in ("PresenceRequest", "ZoneHit", "RegionPresence", "ZonePresence"):
        assert f"message {name} " in text
        for fname, (num, _) in v2[name].items():
            assert f" {fname} = {num};" in text, (name, fname)


# ---- serving on the CPU --------------------------------------------------------------------------

@pytest.mark.parametrize("serve", [True, False])
def test_server_and_client_on_cpu(serve, zone_file, capsys):
    from semantic_segmentation_server_amd import client
    from semantic_segmentation_server_amd.server import Server
    cfg = _on(zone_file, track_regions=True, fps_limit=None) if serve else \
        _cfg(serve_regions=True, serve_zones=True, zones=zone_file, fps_limit=None)
    srv = Server(cfg, max_steps=3).start()
    try:
        srv.producer.join(timeout=120)
        assert srv.producer.steps == 3 and srv.producer.error is None
        target = f"127.0.0.1:{srv.port}"
        if not serve:
            with grpc.insecure_channel(target) as ch:
                with pytest.raises(grpc.RpcError) as e:
                    S.SemanticSegmentationV2Stub(ch).GetZonePresence(P.PresenceRequest(stream_id=0))
            assert e.value.code() == grpc.StatusCode.FAILED_PRECONDITION
            assert client.main(["--target", target, "--presence"]) == 1
            assert srv.hub.presence(0) is None
            return
        m = client.fetch_presence(target, 0)
        eng = srv.engine
        assert (m.width, m.height) == (eng.crop_w, eng.crop_h) and m.frame_id == 2 and m.has_tracks
        assert (m.model_width, m.model_height, m.min_share) == (65, 65, 0.5)
        p = PR.decode(srv.hub.presence(0).words, 4, tracks=True)
        regs = client.fetch_regions(target, 0)
        assert [r.pixels for r in m.regions] == p.P[:, 0].tolist() == [r.pixels for r in regs.regions]
        assert [(r.track_id, r.age) for r in m.regions] == [(r.track_id, r.age) for r in regs.regions]
        for a, r in enumerate(m.regions):
            assert [(h.index, h.pixels, h.dwell) for h in r.zones] == \
                [(z, int(p.P[a, z]), int(p.D[a, z])) for z in (1, 2, 3) if p.P[a, z] > 0]
        capsys.readouterr()
        assert client.main(["--target", target, "--presence", "0"]) == 0
        text = capsys.readouterr().out
        assert "frame 2" in text and "min share 0.500" in text
        if m.regions:
            r = m.regions[0]
            assert f"{r.pixels} px" in text and f"track {r.track_id:>5}" in text
            for h in r.zones:
                assert h.name in text and f"share {h.share:.4f}" in text and f"dwell {h.dwell:>5}" in text
    finally:
        srv.stop(0)


def test_supervised_server_on_cpu(zone_file):
    from semantic_segmentation_server_amd.runtime.supervisor import SupervisedServer
    sup = SupervisedServer(_on(zone_file, max_regions=8), heartbeat_timeout_s=60.0).start()
    try:
        t_end = time.time() + 240
        while sup.hub.presence(0) is None and time.time() < t_end and sup.alive:
            time.sleep(0.05)
        z = sup.hub.presence(0)
        assert z is not None, sup.error
        n = int(z.words[0])
        assert len(z.words) == 4 + PR.unit(4) * n and int(z.words[2]) == 65 and not z.tracks
        with grpc.insecure_channel(f"127.0.0.1:{sup.port}") as ch:
            m = S.SemanticSegmentationV2Stub(ch).GetZonePresence(P.PresenceRequest(stream_id=0))
        assert m.frame_id >= z.frame_id and m.width == 65 and not m.has_tracks and m.min_share == 0.5
        for r in m.regions:
            assert sum(h.pixels for h in r.zones if h.index in (1, 2)) == r.pixels
    finally:
        sup.stop(0)


def test_multi_rank_group_is_rejected(zone_file):
    from semantic_segmentation_server_amd.parallel.dist import DistContext
    from semantic_segmentation_server_amd.parallel.dp import DataParallelPipeline
    from semantic_segmentation_server_amd.parallel.serving import serve_distributed
    from semantic_segmentation_server_amd.runtime.engine import Engine
    eng = Engine(_on(zone_file))
    ctx = DistContext(rank=0, world=2, backend="gloo")  # an initialised world-2 gloo group
    with pytest.raises(ValueError, match="multi-rank"):
        DataParallelPipeline(ctx, eng, 160, 120, 1, "local", None)
    with pytest.raises(ValueError, match="multi-rank"):
        serve_distributed(_on(zone_file, gpus=2, supervise=False))
    # world size 1 is fine, on the CPU too: the presence words ride with the records
    hub = ResultHub(1)
    pipe = DataParallelPipeline(DistContext(), eng, 160, 120, 1, "local", hub, lag=1)
    f = torch.zeros((1, 120, 160, 3), dtype=torch.uint8)
    pipe.prefetch(f)
    pipe.step(frame_ids=[5], ts=[1.0], streams=[0])
    pipe.flush()
    z = hub.presence(0)
    assert z is not None and z.frame_id == 5 and not z.tracks
    p, rt = PR.decode(z.words, 4), RG.decode(hub.regions(0).words)
    assert np.array_equal(p.P[:, 0], rt["pixels"]) and len(z.words) == 4 + PR.unit(4) * p.n
