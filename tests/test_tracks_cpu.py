"""Region tracks on the host: the numpy definition (postprocess/tracks.py) on hand-built
sequences with literal ids and ages, the word functions, and the serving layers that carry the
two extra words. Every comparison is exact."""
import os
from concurrent import futures

import grpc
import numpy as np
import pytest
import torch

from semantic_segmentation_server_amd import config as C
from semantic_segmentation_server_amd.api import proto as P
from semantic_segmentation_server_amd.api import service as S
from semantic_segmentation_server_amd.postprocess import regions as RG
from semantic_segmentation_server_amd.postprocess import tracks as TK
from semantic_segmentation_server_amd.runtime.results import ResultHub

CLASSES = range(1, 21)


def _map(rows):
    return np.array([[int(c) for c in r] for r in rows], np.uint8)


def _bar(width, *spans, rows=1):
    """A rows x width map; spans: (row, x0, x1 inclusive, class)."""
    m = np.zeros((rows, width), np.uint8)
    for y, x0, x1, c in spans:
        m[y, x0:x1 + 1] = c
    return m


def _step(tracker, m, K=8, min_pixels=1):
    """One frame through ``regions.encode`` with the tracker -> [(label, pixels, track_id, age)]
    of the stored regions, in slot order."""
    w = RG.encode(m, m.shape[1], m.shape[0], CLASSES, min_pixels, K, tracker=tracker)
    t = RG.decode(w, tracks=True)
    return [(int(r["label"]), int(r["pixels"]), int(r["track_id"]), int(r["age"])) for r in t]


def _run(maps, q=256, **kw):
    tr = TK.StreamTracker(q)
    return [_step(tr, m, **kw) for m in maps]


# ---- hand-built sequences -----------------------------------------------------------------------

def test_a_translating_blob_keeps_its_id_and_ages():
    maps = []
    for k in range(4):
        m = np.zeros((6, 10), np.uint8)
        m[1:4, 1 + k:4 + k] = 2
        maps.append(m)
    assert _run(maps) == [[(2, 9, 1, a)] for a in (1, 2, 3, 4)]


def test_ids_follow_the_regions_when_the_size_order_flips():
    a = _bar(16, (0, 0, 11, 1), (2, 0, 7, 2), rows=3)   # class 1: 12 px (slot 0), class 2: 8 px (slot 1)
    b = _bar(16, (0, 0, 5, 1), (2, 0, 9, 2), rows=3)    # class 1: 6 px (slot 1), class 2: 10 px (slot 0)
    assert _run([a, b]) == [[(1, 12, 1, 1), (2, 8, 2, 1)], [(2, 10, 2, 2), (1, 6, 1, 2)]]


def test_split_the_larger_overlap_inherits():
    whole = _bar(12, (0, 0, 9, 1))
    split = _bar(12, (0, 0, 5, 1), (0, 7, 9, 1))
    assert _run([whole, split]) == [[(1, 10, 1, 1)], [(1, 6, 1, 2), (1, 3, 2, 1)]]
    # the larger overlap, not the smaller slot: here the right piece is the larger one
    split_r = _bar(12, (0, 0, 2, 1), (0, 4, 9, 1))
    assert _run([whole, split_r]) == [[(1, 10, 1, 1)], [(1, 6, 1, 2), (1, 3, 2, 1)]]
    assert _run([whole, split_r, whole])[2] == [(1, 10, 1, 3)]


def test_merge_takes_the_predecessor_with_the_larger_overlap():
    two = _bar(12, (0, 0, 2, 1), (0, 4, 9, 1))    # 6 px at x 4 .. 9: id 1; 3 px: id 2
    one = _bar(12, (0, 0, 9, 1))
    got = _run([two, two, one])
    assert got[1] == [(1, 6, 1, 2), (1, 3, 2, 2)]
    assert got[2] == [(1, 10, 1, 3)]


def test_a_class_change_breaks_the_track():
    a = _bar(8, (0, 1, 5, 3))
    b = _bar(8, (0, 1, 5, 4))
    assert _run([a, a, b, b]) == [[(3, 5, 1, 1)], [(3, 5, 1, 2)], [(4, 5, 2, 1)], [(4, 5, 2, 2)]]


def test_overlap_just_at_and_just_below_the_threshold():
    q = TK.quantize(0.25)
    assert q == 256
    # 8 px against 8 px, 2 shared: 1024 * 2 = 2048 >= 256 * 8 = 2048 -> eligible
    at = [_bar(16, (0, 0, 7, 1)), _bar(16, (0, 6, 13, 1))]
    assert _run(at, q) == [[(1, 8, 1, 1)], [(1, 8, 1, 2)]]
    # 9 px against 9 px, 2 shared: 2048 < 256 * 9 = 2304 -> a new track
    below = [_bar(16, (0, 0, 8, 1)), _bar(16, (0, 7, 15, 1))]
    assert _run(below, q) == [[(1, 9, 1, 1)], [(1, 9, 2, 1)]]
    # the smaller of the two counts: 9 px against 8 px, 2 shared
    assert _run([_bar(16, (0, 0, 8, 1)), _bar(16, (0, 7, 14, 1))], q)[1] == [(1, 8, 1, 2)]
    # q = 1024: only a region inside the other (or the other inside it) continues
    assert _run([_bar(16, (0, 0, 7, 1)), _bar(16, (0, 2, 5, 1))], 1024)[1] == [(1, 4, 1, 2)]
    assert _run([_bar(16, (0, 0, 7, 1)), _bar(16, (0, 5, 8, 1))], 1024)[1] == [(1, 4, 2, 1)]
    with pytest.raises(ValueError):
        TK.quantize(0.0)
    with pytest.raises(ValueError):
        TK.quantize(1.5)
    assert TK.quantize(1.0) == 1024 and TK.quantize(1e-6) == 1


def test_best_tie_goes_to_the_smaller_predecessor():
    prev = _bar(6, (0, 0, 3, 1), (2, 0, 3, 1), rows=3)          # two 4 px bars: slots 0, 1 by root
    cur = _bar(6, (0, 0, 1, 1), (1, 0, 1, 1), (2, 0, 1, 1), rows=3)  # 6 px, 2 shared with each
    assert _run([prev, cur]) == [[(1, 4, 1, 1), (1, 4, 2, 1)], [(1, 6, 1, 2)]]


def test_winner_tie_goes_to_the_smaller_region_slot():
    prev = _bar(8, (0, 0, 6, 1))
    cur = _bar(8, (0, 0, 2, 1), (0, 4, 6, 1))     # 3 px each, 3 shared each
    assert _run([prev, cur]) == [[(1, 7, 1, 1)], [(1, 3, 1, 2), (1, 3, 2, 1)]]


def test_a_region_pushed_past_K_loses_its_id():
    a = _bar(12, (0, 0, 9, 1), (2, 0, 5, 2), rows=5)
    b = _bar(12, (0, 0, 9, 1), (2, 0, 5, 2), (4, 0, 7, 3), rows=5)
    got = _run([a, b, a], K=2)
    assert got[0] == [(1, 10, 1, 1), (2, 6, 2, 1)]
    assert got[1] == [(1, 10, 1, 2), (3, 8, 3, 1)]      # class 2 is third: not stored
    assert got[2] == [(1, 10, 1, 3), (2, 6, 4, 1)]      # ... and new when it is back
    # the same for a region that drops below min_pixels
    small = _bar(12, (0, 0, 9, 1), (2, 0, 2, 2), rows=5)
    got = _run([a, small, a], min_pixels=4)
    assert got[1] == [(1, 10, 1, 2)] and got[2] == [(1, 10, 1, 3), (2, 6, 3, 1)]


def test_two_interleaved_streams_are_independent_and_reset():
    tr = TK.Trackers(256)
    a, b = _bar(8, (0, 0, 4, 1)), _bar(8, (0, 2, 6, 2))
    assert _step(tr.of(7), a) == [(1, 5, 1, 1)]
    assert _step(tr.of(3), b) == [(2, 5, 1, 1)]
    assert _step(tr.of(7), a) == [(1, 5, 1, 2)]
    assert _step(tr.of(3), a) == [(1, 5, 2, 1)]     # stream 3 saw class 2 there before
    assert _step(tr.of(7), b) == [(2, 5, 2, 1)]
    assert tr.of(7).issued == 2 and tr.of(3).issued == 2
    one = tr.of(7)
    one.reset()
    assert one.issued == 0 and _step(one, b) == [(2, 5, 1, 1)]
    assert _step(tr.of(3), a) == [(1, 5, 2, 2)]     # the other stream's state stays
    tr.reset()
    assert _step(tr.of(3), a) == [(1, 5, 1, 1)]


def test_an_empty_frame_ends_every_track():
    a, none = _bar(8, (0, 0, 4, 1)), np.zeros((1, 8), np.uint8)
    assert _run([a, none, a]) == [[(1, 5, 1, 1)], [], [(1, 5, 2, 1)]]


# ---- the overlap table against a per-pixel loop -------------------------------------------------

@pytest.mark.parametrize("seed", [0, 1, 2])
def test_overlap_equals_a_per_pixel_count(seed):
    rng = np.random.default_rng(seed)
    h, w, K, mp = 11, 13, 5, 2
    coarse = rng.integers(0, 4, (2, 4, 5)).astype(np.uint8)
    maps = np.repeat(np.repeat(coarse, 3, 1), 3, 2)[:, :h, :w].copy()
    flip = rng.random(maps.shape) < 0.1
    maps[flip] = rng.integers(0, 4, int(flip.sum()))
    tabs = [RG.region_table(m, w, h, [1, 2, 3], mp)[:K] for m in maps]
    planes = [TK.slot_plane(m, w, h, [1, 2, 3], mp, K) for m in maps]
    assert all(len(t) >= 2 for t in tabs)
    # the plane by its definition: region a's pixels are those 8-connected to its root
    for m, tab, pl in zip(maps, tabs, planes):
        assert pl.shape == (h * w,) and pl.dtype == np.uint16
        comp = RG.label_components(m, RG.class_mask([1, 2, 3])).reshape(-1)
        for i in range(h * w):
            slots = [a for a in range(len(tab)) if comp[i] == tab["root"][a]]
            assert pl[i] == (slots[0] if slots else TK.NONE)
    want = np.zeros((len(tabs[1]), len(tabs[0])), np.int64)
    for i in range(h * w):
        a, b = int(planes[1][i]), int(planes[0][i])
        if a != TK.NONE and b != TK.NONE and tabs[1]["label"][a] == tabs[0]["label"][b]:
            want[a, b] += 1
    got = TK.overlap(planes[1], planes[0], tabs[1]["label"], tabs[0]["label"])
    assert np.array_equal(got, want) and want.sum() > 0
    # best / winner / matched by plain loops
    q = 256
    best, matched = TK.associate(got, tabs[1]["pixels"], tabs[0]["pixels"], q)
    n, m_ = want.shape
    wbest = []
    for a in range(n):
        el = [(int(want[a, b]), -b) for b in range(m_) if want[a, b] > 0 and
              1024 * int(want[a, b]) >= q * min(int(tabs[1]["pixels"][a]), int(tabs[0]["pixels"][b]))]
        wbest.append(-max(el)[1] if el else -1)
    wmatched = []
    for a in range(n):
        if wbest[a] < 0:
            wmatched.append(False)
            continue
        rivals = [(int(want[x, wbest[a]]), -x) for x in range(n) if wbest[x] == wbest[a]]
        wmatched.append(-max(rivals)[1] == a)
    assert best.tolist() == wbest and matched.tolist() == wmatched


def test_batch_tables():
    pred, stream, last = TK.batch_tables([2, 1])
    assert (pred.tolist(), stream.tolist(), last.tolist()) == ([-1, 0, -1], [0, 0, 1], [1, 2])
    pred, stream, last = TK.batch_tables([1, 0])
    assert (pred.tolist(), stream.tolist(), last.tolist()) == ([-1], [0], [0, -1])
    assert TK.batch_tables([4])[0].tolist() == [-1, 0, 1, 2]
    with pytest.raises(ValueError):
        TK.batch_tables([0, 0])


# ---- word functions -----------------------------------------------------------------------------

def _two_frames():
    a = _map(["1100", "1100", "0022"])
    b = _map(["1100", "1000", "0222"])
    return a, b


@pytest.mark.parametrize("conf", [False, True])
@pytest.mark.parametrize("tracks", [False, True])
def test_encode_decode_round_trip(conf, tracks):
    a, b = _two_frames()
    cmap = (np.arange(12, dtype=np.uint8) * 20).reshape(3, 4)
    tr = TK.StreamTracker() if tracks else None
    kw = dict(conf=cmap) if conf else {}
    if tracks:
        kw["tracker"] = tr
    rw = 6 + conf + 2 * tracks
    assert RG.words_per_region(conf, tracks) == rw
    K = 3
    w0 = RG.encode(a, 4, 3, CLASSES, 1, K, **kw)
    w1 = RG.encode(b, 4, 3, CLASSES, 1, K, **kw)
    assert w0.shape == w1.shape == (4 + rw * K,)
    assert RG.used_words(w1, conf=conf, tracks=tracks) == 4 + rw * 2
    t = RG.decode(w1, conf=conf, tracks=tracks)
    assert t["label"].tolist() == [1, 2] and t["pixels"].tolist() == [3, 3]
    assert t["track_id"].tolist() == ([1, 2] if tracks else [0, 0])
    assert t["age"].tolist() == ([2, 2] if tracks else [0, 0])
    if conf:
        assert t["sum_conf"].tolist() == [int(cmap[b == 1].sum()), int(cmap[b == 2].sum())]
    again = np.zeros_like(w1)
    again[:4] = w1[:4]
    again[4:4 + rw * 2] = RG.pack(t, conf, tracks).reshape(-1)
    assert np.array_equal(again, w1)
    # the other words are those of the form without tracks
    plain = RG.encode(b, 4, 3, CLASSES, 1, K, **({"conf": cmap} if conf else {}))
    base = 6 + conf
    assert np.array_equal(w1[:4], plain[:4])
    assert np.array_equal(w1[4:].reshape(K, rw)[:, :base], plain[4:].reshape(K, base))


def test_the_old_calls_give_the_old_words():
    a, _ = _two_frames()
    w = RG.encode(a, 4, 3, CLASSES, 1, 4)  # as before: six words, nothing appended
    assert w.shape == (4 + 6 * 4,) and RG.words_per_region() == 6 and RG.words_per_region(True) == 7
    want = np.zeros(28, np.uint32)
    want[:4] = (2, 12, 4, 3)
    want[4:10] = ((1 << 24) | 0, 4, 2, 2, 0 | (0 << 16), 1 | (1 << 16))
    want[10:16] = ((2 << 24) | 10, 2, 5, 4, 2 | (2 << 16), 3 | (2 << 16))
    assert np.array_equal(w, want)
    assert RG.used_words(w) == 16 and RG.used_words(w, 4) == 16
    t = RG.decode(w)
    assert t["track_id"].tolist() == [0, 0] and t["age"].tolist() == [0, 0]
    assert RG.pack(t).shape == (2, 6) and RG.pack(t, True).shape == (2, 7)
    sentinel = RG.encode(a, 4, 3, CLASSES, 1, 4, np.full(28, 0xABCD, np.uint32))  # out, positionally
    assert np.array_equal(sentinel[:16], want[:16]) and (sentinel[16:] == 0xABCD).all()
    with pytest.raises(ValueError):
        RG.encode(a, 4, 3, CLASSES, 1, 4, out=np.zeros(28, np.uint32), tracker=TK.StreamTracker())


# ---- hub, channel, RPC --------------------------------------------------------------------------

def _track_rows(maps, K, conf=None):
    tr = TK.StreamTracker()
    return np.stack([RG.encode(m, m.shape[1], m.shape[0], CLASSES, 1, K, tracker=tr,
                               **({"conf": conf} if conf is not None else {})) for m in maps])


def test_hub_keeps_the_latest_rows_per_stream_with_tracks():
    a, b = _two_frames()
    rows = _track_rows([a, b, a], 4)
    assert rows.shape == (3, 4 + 8 * 4)
    hub = ResultHub(2)
    hub.push_regions(rows.view(np.int32), np.array([[10, 0, 1.0], [11, 1, 1.5], [12, 0, 2.0]]), tracks=True)
    r0, r1 = hub.regions(0), hub.regions(1)
    assert (r0.frame_id, r1.frame_id, r0.tracks, r1.tracks, r0.conf) == (12, 11, True, True, False)
    assert np.array_equal(r0.words, rows[2][:4 + 16]) and np.array_equal(r1.words, rows[1][:4 + 16])
    assert RG.decode(r0.words, tracks=True)["age"].tolist() == [3, 3]
    plain = np.stack([RG.encode(m, 4, 3, CLASSES, 1, 4) for m in (a, b)])
    hub.push_regions(plain, np.array([[13, 0, 3.0], [14, 1, 3.5]]))  # as before the flag existed
    assert not hub.regions(0).tracks and len(hub.regions(0).words) == 4 + 12
    cmap = np.full((3, 4), 200, np.uint8)
    both = _track_rows([a], 4, conf=cmap)
    hub.push_regions(both, np.array([[15, 1, 4.0]]), conf=True, tracks=True)
    r = hub.regions(1)
    assert r.conf and r.tracks and len(r.words) == 4 + 9 * 2


@pytest.mark.parametrize("conf", [False, True])
def test_supervisor_channel_round_trip(conf):
    from semantic_segmentation_server_amd.runtime.supervisor import _RingHub, _WordChannel
    a, b = _two_frames()
    rows = _track_rows([a, b], 4, conf=np.full((3, 4), 9, np.uint8) if conf else None)
    unit = 8 + conf
    ch = _WordChannel(streams=2, cap=4, first=4, unit=unit)
    try:
        peer = _WordChannel(name=ch.name)
        assert peer.unit == unit
        hub = _RingHub(None, None, peer)
        hub.push_regions(rows, np.array([[7, 4, 1.0], [8, 4, 2.0]]), conf=conf, tracks=True)
        got = ch.pull()
        assert [(s, f, t) for s, f, t, _ in got] == [(4, 8, 2.0)]
        assert np.array_equal(got[0][3], rows[1][:4 + unit * 2])
        peer.close()
    finally:
        ch.close()


def test_supervisor_channel_unit_follows_the_config():
    from semantic_segmentation_server_amd.runtime import supervisor as SV
    import inspect
    src = inspect.getsource(SV.SupervisedServer._pull)
    assert "tracks=" in src
    hub = ResultHub(1)
    a, b = _two_frames()
    rows = _track_rows([a, b], 4)
    hub.put_regions(0, 3, 1.0, rows[1][:20], conf=False, tracks=True)
    assert hub.regions(0).tracks and not hub.regions(0).conf


class _Ctx:
    code = None

    def set_code(self, c):
        self.code = c

    def set_details(self, d):
        self.details = d


def test_status_codes_unchanged():
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
    a, b = _two_frames()
    hub.push_regions(_track_rows([a, b], 4), np.array([[1, 0, 0.5], [2, 0, 0.6]]), tracks=True)
    ctx = _Ctx()
    m = on.GetClassRegions(P.RegionRequest(stream_id=0), ctx)
    assert ctx.code is None and m.has_tracks and not m.has_confidence
    assert [(r.class_id, r.pixels, r.track_id, r.age) for r in m.regions] == [(1, 3, 1, 2), (2, 3, 2, 2)]
    # without the words the fields stay 0 / false
    hub.push_regions(np.stack([RG.encode(a, 4, 3, CLASSES, 1, 4)]), np.array([[3, 0, 0.7]]))
    m = on.GetClassRegions(P.RegionRequest(stream_id=0), _Ctx())
    assert not m.has_tracks and [(r.track_id, r.age) for r in m.regions] == [(0, 0), (0, 0)]


def test_loopback_rpc_serves_the_fields():
    a, b = _two_frames()
    cmap = np.full((3, 4), 255, np.uint8)
    hub = ResultHub(2)
    hub.push_regions(_track_rows([a, b, b], 8, conf=cmap), np.array([[40, 1, 1.0], [41, 1, 2.0], [42, 1, 123.25]]),
                     conf=True, tracks=True)
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
            assert m.has_tracks and m.has_confidence and m.total_regions == 2
            assert [(r.class_id, r.track_id, r.age, r.confidence) for r in m.regions] == \
                [(1, 1, 3, 1.0), (2, 2, 3, 1.0)]
            with pytest.raises(grpc.RpcError) as e:
                stub.GetClassRegions(P.RegionRequest(stream_id=0))
            assert e.value.code() == grpc.StatusCode.UNAVAILABLE
    finally:
        server.stop(0)


def test_proto_fields_and_the_readable_proto():
    v2 = P.v2_file_descriptor()
    msgs = {m.name: {f.name: (f.number, f.type) for f in m.field} for m in v2.message_type}
    F = type(v2.message_type[0].field[0])
    assert msgs["ClassRegion"]["track_id"] == (12, F.TYPE_UINT32)
    assert msgs["ClassRegion"]["age"] == (13, F.TYPE_UINT32)
    assert msgs["ClassRegions"]["has_tracks"] == (12, F.TYPE_BOOL)
    assert "track_id" not in {f.name for m in P.v1_file_descriptor().message_type for f in m.field}
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                        "semantic_segmentation_server_amd", "api", "sem_seg_server_v2.proto")
    with open(path) as f:
        text = f.read()
    for line in ("uint32 track_id = 12;", "uint32 age = 13;", "bool has_tracks = 12;"):
        assert line in text


def test_client_prints_the_columns_only_with_tracks(capsys):
    from semantic_segmentation_server_amd import client
    r = P.ClassRegion(label="car", class_id=7, pixels=5, track_id=31, age=4)
    client.print_regions(P.ClassRegions(regions=[r], total_regions=1, has_tracks=True))
    out = capsys.readouterr().out
    assert "track    31" in out and "age     4" in out
    client.print_regions(P.ClassRegions(regions=[r], total_regions=1))
    assert "track" not in capsys.readouterr().out


# ---- configuration and engine -------------------------------------------------------------------

def _cfg(**kw):
    base = dict(backend="torch", device="cpu", input_size=65, batch=1, port=0, host="127.0.0.1",
                min_area_ratio=0.0005, fps_limit=200.0, log_level="WARNING")
    base.update(kw)
    return C.Config(**base)


def test_cli_flags_and_refusals():
    cfg = C.parse(["--serve_regions", "--track_regions", "--track_min_overlap", "0.5"])
    assert cfg.track_regions and cfg.track_min_overlap == 0.5
    d = C.parse([])
    assert (d.track_regions, d.track_min_overlap) == (False, 0.25)
    with pytest.raises(ValueError, match="--track_regions requires --serve_regions"):
        C.parse(["--track_regions"])
    for bad in ("0", "1.5", "-0.1"):
        with pytest.raises(ValueError, match="track_min_overlap"):
            C.parse(["--serve_regions", "--track_regions", "--track_min_overlap", bad])
    assert C.parse(["--serve_regions", "--track_min_overlap", "1.0", "--track_regions"]).track_min_overlap == 1.0


def test_refused_where_a_stream_is_not_post_processed_in_order_with_one_state(monkeypatch):
    from semantic_segmentation_server_amd.parallel.dist import DistContext
    from semantic_segmentation_server_amd.parallel.dp import DataParallelPipeline
    from semantic_segmentation_server_amd.parallel.serving import serve_distributed
    from semantic_segmentation_server_amd.runtime.engine import Engine
    from semantic_segmentation_server_amd.runtime.multistream import StreamGroup
    eng = Engine(_cfg(serve_regions=True, track_regions=True))
    assert eng.region_words == 8 and eng.track_q == 256 and eng.track_streams == 1
    assert Engine(_cfg(serve_regions=True, track_regions=True, serve_confidence=True)).region_words == 9
    plain = Engine(_cfg(serve_regions=True))
    assert plain.region_words == 6 and not plain.track_regions and plain.track_streams == 0
    ctx = DistContext(rank=0, world=2, backend="gloo")
    with pytest.raises(ValueError, match="track_regions"):
        DataParallelPipeline(ctx, eng, 160, 120, 1, "local", None)
    with pytest.raises(ValueError, match="track_regions"):
        serve_distributed(_cfg(serve_regions=True, track_regions=True, gpus=2, supervise=False))
    with pytest.raises(ValueError, match="track_regions"):
        StreamGroup(_cfg(serve_regions=True, track_regions=True), torch.device("cpu"), 2)
    # SSA_MODEL_PARTS > 1 is refused where the parts would be made: bind_inputs on a GPU engine
    import inspect
    assert "SSA_MODEL_PARTS" in inspect.getsource(Engine.bind_inputs)


def test_the_layout_check_names_the_flag():
    from semantic_segmentation_server_amd.runtime.engine import Engine
    eng = Engine(_cfg(serve_regions=True, track_regions=True, streams=2, batch=3))
    assert eng.track_layout(3) == [0, 0, 1] and eng.track_layout(4) == [0, 0, 1, 1]
    eng.check_track_streams([5, 5, 9], 3)
    eng.check_track_streams([5, 5, 9], 3)
    for bad in ([5, 9, 5], [9, 9, 5], [5, 5, 5], [5, 5], 5):
        with pytest.raises(ValueError, match="--track_regions"):
            eng.check_track_streams(bad, 3)
    eng.reset_tracks()
    eng.check_track_streams([9, 9, 5], 3)  # a new run may number its streams anew


def test_cpu_engine_sequence_equals_the_tracker_on_its_own_labels():
    from semantic_segmentation_server_amd.runtime.engine import Engine
    from semantic_segmentation_server_amd.runtime.sources import SyntheticSource
    eng = Engine(_cfg(serve_regions=True, track_regions=True, batch=3, streams=2,
                      region_min_area_ratio=0.001, track_min_overlap=0.5))
    src = SyntheticSource(160, 120, pool=12, seed=3)
    oracle = {5: TK.StreamTracker(512), 9: TK.StreamTracker(512)}
    streams = [5, 5, 9]
    aged = 0
    for k in range(4):
        f, _, _ = src.read_batch(3)
        if k == 2:
            f = prev  # a repeated batch: every region continues
        prev = f
        eng.step(f, [3 * k, 3 * k + 1, 3 * k + 2], [0.0] * 3, streams)
        with torch.no_grad():
            lab = eng._infer_eager(torch.from_numpy(f)).numpy()
        assert eng.regions.shape == (3, 4 + 8 * 64) and eng.regions.dtype == np.uint32
        for b in range(3):
            want = RG.encode(lab[b], eng.crop_w, eng.crop_h, RG.default_classes(21), eng.region_min_pixels,
                             64, tracker=oracle[streams[b]])
            assert np.array_equal(eng.regions[b], want), (k, b)
            aged += int((RG.decode(want, tracks=True)["age"] > 1).sum())
    assert aged > 0
    eng.reset_tracks()
    eng.step(prev, [0, 1, 2], [0.0] * 3, streams)
    t = RG.decode(eng.regions[2], tracks=True)
    assert len(t) and t["track_id"].tolist() == list(range(1, len(t) + 1)) and (t["age"] == 1).all()
    # flag off: the rows and the records of the same frames are those of the parent's code path
    off = Engine(_cfg(serve_regions=True, batch=3, streams=2, region_min_area_ratio=0.001))
    recs_off = off.step(prev, [0, 1, 2], [0.0] * 3, streams)
    assert off.regions.shape == (3, 4 + 6 * 64) and off._trackers is None
    on = eng.regions[:, 4:].reshape(3, 64, 8)
    assert np.array_equal(off.regions[:, :4], eng.regions[:, :4])
    assert np.array_equal(off.regions[:, 4:].reshape(3, 64, 6), on[:, :, :6])


def test_server_on_cpu_serves_tracks():
    from semantic_segmentation_server_amd.server import Server
    srv = Server(_cfg(serve_regions=True, track_regions=True, fps_limit=None,
                      region_min_area_ratio=0.001), max_steps=3).start()
    try:
        srv.producer.join(timeout=120)
        assert srv.producer.steps == 3 and srv.producer.error is None
        with grpc.insecure_channel(f"127.0.0.1:{srv.port}") as ch:
            m = S.SemanticSegmentationV2Stub(ch).GetClassRegions(P.RegionRequest(stream_id=0))
        r = srv.hub.regions(0)
        assert r.tracks and m.has_tracks and m.frame_id == 2
        tab = RG.decode(r.words, tracks=True)
        assert [(x.track_id, x.age) for x in m.regions] == list(zip(tab["track_id"].tolist(), tab["age"].tolist()))
        assert len(tab) and (tab["track_id"] >= 1).all() and (tab["age"] >= 1).all() and (tab["age"] <= 3).all()
    finally:
        srv.stop(0)


def test_pipeline_on_cpu_carries_the_wider_rows():
    from semantic_segmentation_server_amd.parallel.dist import DistContext
    from semantic_segmentation_server_amd.parallel.dp import DataParallelPipeline
    from semantic_segmentation_server_amd.runtime.engine import Engine
    eng = Engine(_cfg(serve_regions=True, track_regions=True, region_min_area_ratio=0.001))
    hub = ResultHub(1)
    pipe = DataParallelPipeline(DistContext(), eng, 160, 120, 1, "local", hub, lag=1)
    from semantic_segmentation_server_amd.runtime.sources import SyntheticSource
    f = torch.from_numpy(SyntheticSource(160, 120, pool=1, seed=3).read_batch(1)[0].copy())
    for k in range(3):
        pipe.prefetch(f)
        pipe.step(frame_ids=[5 + k], ts=[1.0], streams=[0])
    pipe.flush()
    r = hub.regions(0)
    t = RG.decode(r.words, tracks=True)
    assert r.tracks and r.frame_id == 7 and len(t) and (t["age"] == 3).all()
    assert t["track_id"].tolist() == list(range(1, len(t) + 1))
