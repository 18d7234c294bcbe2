"""Zone events on the host: the definition (postprocess/events.py) by hand and over the sequences of
tests/presence_cases.py, the hub's log, the supervisor's ring, the v2 GetZoneEvents servicer, the
config and the CPU engine path. Every comparison of words is exact.
"""
import json
import os

import grpc
import numpy as np
import pytest
import torch

import event_cases as EC
import presence_cases as PC
from semantic_segmentation_server_amd import config as C
from semantic_segmentation_server_amd.api import proto as P
from semantic_segmentation_server_amd.api import service as S
from semantic_segmentation_server_amd.postprocess import events as EV
from semantic_segmentation_server_amd.postprocess import presence as PR
from semantic_segmentation_server_amd.runtime import results as RS
from semantic_segmentation_server_amd.runtime.results import EVENT_DTYPE, ResultHub

BIG = 0xFFFFFFFF


def _w0(slot, r, kind, edge):
    return slot | r << 8 | kind << 16 | edge << 24


def _events(words):
    """[(w0, w1, w2, w3)] of the stored events of one frame."""
    k = (EV.used_words(words) - 4) // 4
    return [tuple(int(v) for v in words[4 + 4 * j:8 + 4 * j]) for j in range(k)]


# ---- the definition by hand ----------------------------------------------------------------------

def test_hand_case_every_kind_of_edge_in_order():
    """K = 4, R = 3. prev: tracks 5, 6, 7, 8. cur: 7 and 5 continue (in a new order), 6 and 8 end,
    9 is born inside zone 1."""
    K, R = 4, 3
    f = lambda lab, root: (lab << 24) | root
    prev = EC.row(K, R, [5, 6, 7, 8], [[4, 2, 0], [9, 0, 3], [2, 2, 2], [1, 0, 0]],
                  first=[f(1, 10), f(2, 20), f(3, 30), f(4, 40)])
    cur = EC.row(K, R, [7, 9, 5], [[3, 0, 3], [1, 1, 0], [5, 3, 1]],
                 P=[[50, 0, 20], [30, 30, 0], [80, 60, 11]], first=[f(3, 31), f(5, 50), f(1, 11)])
    w = EV.events_between(prev, cur, R, 16)
    assert w[:4].tolist() == [7, EC.CW * EC.CH, EC.CW, EC.CH] and len(w) == EV.frame_words(16) == 68
    assert _events(w) == [
        # LEAVEs ascending in (b, r): track 6 ends inside zone 2 (edge), 7 leaves zone 1 and goes
        # on, 8 ends
        (_w0(1, 0, 2, 1), 6, f(2, 20), 9), (_w0(1, 2, 2, 1), 6, f(2, 20), 3),
        (_w0(2, 1, 2, 0), 7, f(3, 30), 2), (_w0(3, 0, 2, 1), 8, f(4, 40), 1),
        # ENTERs ascending in (a, r): 9 is born inside zone 1 (edge on both), 5 enters zone 2
        (_w0(1, 0, 1, 1), 9, f(5, 50), 30), (_w0(1, 1, 1, 1), 9, f(5, 50), 30),
        (_w0(2, 2, 1, 0), 5, f(1, 11), 11)]
    assert not w[4 + 4 * 7:].any()
    d = EV.decode(w)
    assert d["kind"].tolist() == [2, 2, 2, 2, 1, 1, 1] and d["zone"].tolist() == [0, 2, 1, 0, 0, 1, 2]
    assert d["edge"].tolist() == [1, 1, 0, 1, 1, 1, 0] and d["label"].tolist() == [2, 2, 3, 4, 5, 5, 1]
    assert d["root"].tolist() == [20, 20, 30, 40, 50, 50, 11] and d["value"].tolist() == [9, 3, 2, 1, 30, 30, 11]
    assert EV.used_words(w) == 4 + 4 * 7


def test_re_entry_and_a_split_whose_keeper_keeps_its_zone():
    R, K = 2, 4
    frames = [EC.row(K, R, [1], [[1, 1]]), EC.row(K, R, [1], [[2, 0]]), EC.row(K, R, [1], [[3, 1]]),
              # a split: the piece that keeps id 1 stays in the zone, the other is a fresh track
              EC.row(K, R, [1, 2], [[4, 2], [1, 1]])]
    ev = [_events(w) for w in EC.oracle(frames, R, 8)]
    assert [[(e[0] >> 16 & 0xFF, e[0] >> 8 & 0xFF, e[0] >> 24, e[1], e[3]) for e in f] for f in ev] == [
        [(1, 0, 1, 1, frames[0][4 + 2]), (1, 1, 1, 1, frames[0][4 + 3])],   # birth, inside the zone
        [(2, 1, 0, 1, 1)],                                                  # leaves after 1 frame
        [(1, 1, 0, 1, frames[2][4 + 3])],                                   # re-entry: no edge
        [(1, 0, 1, 2, frames[3][4 + 6 + 2]), (1, 1, 1, 2, frames[3][4 + 6 + 3])]]  # the keeper: no event


def test_no_predecessor_after_reset_and_empty_frames():
    R, K = 3, 4
    cur = EC.row(K, R, [4, 9], [[3, 0, 2], [BIG, BIG, 1]])
    for prev in (None, EC.row(K, R, [], np.zeros((0, R)))):
        w = EV.events_between(prev, cur, R, 8)
        assert w[0] == 1 and _events(w) == [(_w0(1, 2, 1, 0), 9, int(cur[4 + 8]), int(cur[4 + 8 + 2 + 2]))]
    st = EV.StreamEvents(8)
    assert np.array_equal(st.update(PR.decode(cur, R, True)), w)
    gone = st.update(PR.decode(EC.row(K, R, [], np.zeros((0, R))), R, True))   # cur.n = 0: everything ends
    assert gone[0] == 5 and all(e[0] >> 16 & 0xFF == 2 and e[0] >> 24 == 1 for e in _events(gone))
    assert [e[3] for e in _events(gone)] == [3, 2, BIG, BIG, 1]               # D = 0xFFFFFFFF is a dwell
    st.reset()
    assert np.array_equal(st.update(PR.decode(cur, R, True)), w)
    ev = EV.Events(8)
    assert ev.of(3) is ev.of(3) and ev.of(3) is not ev.of(4) and ev.of(3).E == 8
    ev.of(3).update(PR.decode(cur, R, True))
    ev.reset()
    assert ev.of(3).prev is None


@pytest.mark.parametrize("total", [3, 4, 5])
def test_truncation_keeps_the_true_count(total):
    """E = 4 with E - 1, E and E + 1 events."""
    K, R, E = 4, 3, 4
    cand = [0, 5, 11, 12, 19][:total]
    prev, cur = EC.events_at(K, R, 4, 4, cand)
    full = EV.events_between(prev, cur, R, 16)
    w = EV.events_between(prev, cur, R, E)
    assert full[0] == w[0] == total and len(w) == 20
    k = min(total, E)
    assert np.array_equal(w[4:4 + 4 * k], full[4:4 + 4 * k]) and not w[4 + 4 * k:].any()
    assert EV.used_words(w) == 4 + 4 * k and len(EV.decode(w)) == k
    out = np.full(20, EC.SENT, np.uint32)
    assert EV.events_between(prev, cur, R, E, out=out) is out and np.array_equal(out, w)


def test_events_at_places_exactly_the_candidates():
    K, R, pn, cn = 12, 6, 11, 9
    cand = EC.boundary_candidates(pn, cn, R)
    assert cand == [0, 63, 64, 65, 66, 119]
    prev, cur = EC.events_at(K, R, pn, cn, cand)
    d = EV.decode(EV.events_between(prev, cur, R, 64))
    got = [int(e["slot"]) * R + int(e["zone"]) + (pn * R if e["kind"] == 1 else 0) for e in d]
    assert got == cand


def test_one_row_gives_births_and_ends_only():
    rng = np.random.default_rng(5)
    rows = EC.random_sequence(rng, 6, 1, 12)
    seen = 0
    for w in EC.oracle(rows, 1, 64):
        d = EV.decode(w)
        assert (d["zone"] == 0).all()
        seen += len(d)
    assert seen > 0
    prev, cur = EC.all_flip(5, 1)
    d = EV.decode(EV.events_between(prev, cur, 1, 64))
    assert d["kind"].tolist() == [2] * 5 + [1] * 5 and d["edge"].all()


def test_all_flip_worst_case_counts():
    prev, cur = EC.all_flip(256, 33)
    w = EV.events_between(prev, cur, 33, 4096)
    d = EV.decode(w)
    assert w[0] == 2 * 8448 and len(d) == 4096 and (d["kind"] == 2).all() and (d["value"] == 7).all()
    assert d["slot"][-1] == 4095 // 33 and d["zone"][-1] == 4095 % 33


def test_check_geometry_and_helpers():
    for E in (1, 64, 4096):
        EV.check_geometry(E)
        assert EV.frame_words(E) == 4 + 4 * E
    for E in (0, 4097, -1):
        with pytest.raises(ValueError, match="--max_events"):
            EV.check_geometry(E)
    with pytest.raises(ValueError):
        EV.events_between(None, EC.row(2, 2, [1], [[1, 1]]), 2, 4, out=np.zeros(19, np.uint32))
    with pytest.raises(ValueError):
        EV.decode(np.zeros(3, np.uint32))


# ---- the sequences of the presence tests ---------------------------------------------------------

def test_the_presence_sequences_through_the_definition():
    o0, o1 = PC.sequence_oracles()
    ev0 = [EV.decode(w) for w in EC.oracle([p for _, p in o0], 4, 64)]
    t1 = [e[e["track_id"] == 1] for e in ev0]
    born = t1[0]
    assert (born["kind"] == 1).all() and born["zone"].tolist()[:2] == [0, 1] and born["edge"].all()
    leave = t1[5]
    assert leave["kind"].tolist() == [2] and leave["zone"].tolist() == [1] and leave["value"].tolist() == [5]
    assert not leave["edge"][0]
    assert [(int(e["kind"]), int(e["zone"])) for e in t1[6]] == [(1, 1)]         # the re-entry
    for k in (1, 2, 3, 4):   # inside "left" all along (at frame 4, exactly half inside, it also enters "right")
        assert not (t1[k]["zone"] == 1).any() and not (t1[k]["zone"] == 0).any()
    assert [(int(e["kind"]), int(e["zone"]), int(e["value"])) for e in t1[4]] == [(1, 2, 50)]
    fresh = ev0[7][(ev0[7]["kind"] == 1) & (ev0[7]["zone"] == 0)]               # the smaller piece of the split
    assert len(fresh) == 1 and fresh["edge"][0] == 1 and fresh["track_id"][0] != 1 and fresh["value"][0] == 30
    assert not ((ev0[7]["track_id"] == 1) & (ev0[7]["zone"] == 0)).any()        # the keeper goes on
    total = sum(int(w[0]) for w in EC.oracle([p for _, p in o1], 4, 64))
    assert total > 0


# ---- hub -----------------------------------------------------------------------------------------

def _frame(E, events, n=None):
    w = np.zeros(EV.frame_words(E), np.uint32)
    w[:4] = (len(events) if n is None else n, 1200, 40, 30)
    for j, e in enumerate(events[:E]):
        w[4 + 4 * j:8 + 4 * j] = e
    return w


def _ev(k, zone=1, kind=1):
    return (_w0(k % 200, zone, kind, 0), 100 + k, (3 << 24) | k, 7 + k)


def test_hub_log_sequence_numbers_overflow_truncation_and_epoch():
    hub = ResultHub(2, event_log=8)
    assert hub.events_after(0, 0, 100)[1:] == (0, 0) and len(hub.events_after(0, 0)[0]) == 0
    E = 4
    rows = np.stack([_frame(E, [_ev(0), _ev(1)]), _frame(E, []), _frame(E, [_ev(2)]),
                     _frame(E, [_ev(3), _ev(4), _ev(5), _ev(6)], n=7)])
    meta = np.array([[10, 0, 1.0], [10, 1, 1.5], [11, 1, 2.5], [11, 0, 2.0]])
    hub.push_events(rows.view(np.int32), meta)
    ev, nxt, lost = hub.events_after(0, 0, 100)
    assert ev.dtype == EVENT_DTYPE and ev["seq"].tolist() == [1, 2, 3, 4, 5, 6] and (nxt, lost) == (6, 0)
    assert ev["frame_id"].tolist() == [10, 10, 11, 11, 11, 11] and ev["ts"].tolist() == [1.0, 1.0, 2.0, 2.0, 2.0, 2.0]
    assert ev["w1"].tolist() == [100, 101, 103, 104, 105, 106] and (ev["epoch"] == 0).all() and (ev["stream"] == 0).all()
    assert hub.events_truncated(0) == 3 and hub.events_truncated(1) == 0
    ev1, nxt1, _ = hub.events_after(1, 0, 100)
    assert ev1["seq"].tolist() == [1] and ev1["frame_id"].tolist() == [11] and nxt1 == 1
    # the cursor and the limit
    ev, nxt, lost = hub.events_after(0, 2, 3)
    assert ev["seq"].tolist() == [3, 4, 5] and (nxt, lost) == (5, 0)
    assert hub.events_after(0, 6, 10)[1:] == (6, 0) and len(hub.events_after(0, 6, 10)[0]) == 0
    # overflow of the ring of 8: seq 7 .. 11 push 1 .. 3 out
    hub.bump_epoch([0])
    hub.push_events(np.stack([_frame(E, [_ev(7), _ev(8), _ev(9)]), _frame(E, [_ev(10), _ev(11)])]),
                    np.array([[12, 0, 3.0], [13, 0, 4.0]]))
    ev, nxt, lost = hub.events_after(0, 1, 100)
    assert ev["seq"].tolist() == list(range(4, 12)) and (nxt, lost) == (11, 2)
    assert ev["epoch"].tolist() == [0, 0, 0, 1, 1, 1, 1, 1] and ev["frame_id"].tolist()[-2:] == [13, 13]
    assert hub.events_after(0, 5, 100)[2] == 0 and hub.events_truncated(0) == 3
    ev, nxt, lost = hub.events_after(0, 0, 2)
    assert ev["seq"].tolist() == [4, 5] and (nxt, lost) == (5, 3)
    # the hub's own copy
    ev["w1"][:] = 0
    assert hub.events_after(0, 3, 1)[0]["w1"].tolist() == [104]
    # one frame with more events than the log holds: the newest stay
    big = ResultHub(1, event_log=4)
    big.push_events(_frame(6, [_ev(k) for k in range(6)])[None], np.array([[1, 0, 0.5]]))
    ev, nxt, lost = big.events_after(0, 0, 10)
    assert ev["seq"].tolist() == [3, 4, 5, 6] and (nxt, lost) == (6, 2)
    with pytest.raises(ValueError, match="--event_log"):
        ResultHub(1, event_log=0)


def test_a_quiet_push_does_no_per_frame_work(monkeypatch):
    calls = []
    real = RS.event_rows
    monkeypatch.setattr(RS, "event_rows", lambda *a, **k: calls.append(1) or real(*a, **k))
    hub = ResultHub(1)
    monkeypatch.setattr(hub, "push_event_rows", lambda ev: calls.append(2))
    quiet = np.stack([_frame(4, [])] * 32)

    class Meta:  # any per-frame read of the metadata would be seen
        def __getitem__(self, k):
            calls.append(3)
            raise AssertionError("metadata read on a quiet step")

    hub.push_events(quiet, Meta())
    assert calls == []
    hub.push_events(np.stack([_frame(4, []), _frame(4, [_ev(1)])]), np.array([[1, 0, 0.0], [2, 0, 0.0]]))
    assert calls == [1, 2]


# ---- supervisor ring -----------------------------------------------------------------------------

def test_supervisor_ring_round_trips_events_across_a_wrap():
    from semantic_segmentation_server_amd.runtime.supervisor import _RecordRing, _RingHub
    ring = _RecordRing(8, dtype=EVENT_DTYPE)
    assert _RecordRing.__init__.__defaults__[-1] is RS.RECORD_DTYPE
    try:
        peer = _RecordRing(name=ring.name, dtype=EVENT_DTYPE)
        worker, hub = _RingHub(None, events=peer), ResultHub(2, event_log=64)
        E, sent = 4, []
        for step in range(5):                     # 5 pushes of 3 rows through a ring of 8: it wraps
            rows = np.stack([_frame(E, [_ev(10 * step), _ev(10 * step + 1)]), _frame(E, []),
                             _frame(E, [_ev(10 * step + 2)])])
            meta = np.array([[step, 0, step + 0.25], [step, 1, step + 0.5], [step + 100, 1, step + 0.75]])
            worker.push_events(rows, meta)
            sent.append((rows, meta))
            hub.push_event_rows(ring.pull())
        assert ring.drops == 0 and int(ring.hdr[0]) == 15
        ev, nxt, lost = hub.events_after(0, 0, 100)
        assert ev["seq"].tolist() == list(range(1, 11)) and ev["w1"].tolist() == [100 + 10 * s + j for s in range(5) for j in (0, 1)]
        assert ev["frame_id"].tolist() == [s for s in range(5) for _ in (0, 1)] and ev["ts"][3] == 1.25
        ev1, _, _ = hub.events_after(1, 0, 100)
        assert ev1["frame_id"].tolist() == [100, 101, 102, 103, 104] and ev1["w1"].tolist() == [102 + 10 * s for s in range(5)]
        # a quiet batch pushes nothing; a truncated frame carries its count
        worker.push_events(np.stack([_frame(E, [])] * 3), sent[0][1])
        assert int(ring.hdr[0]) == 15
        worker.push_events(_frame(E, [_ev(k) for k in range(4)], n=9)[None], np.array([[7, 0, 9.0]]))
        hub.push_event_rows(ring.pull())
        assert hub.events_truncated(0) == 5 and hub.events_after(0, 10, 100)[0]["seq"].tolist() == [11, 12, 13, 14]
        _RingHub(None).push_events(sent[0][0], sent[0][1])   # no ring: dropped
        peer.close()
    finally:
        ring.close()


# ---- servicer ------------------------------------------------------------------------------------

class _Ctx:
    code = None

    def set_code(self, c):
        self.code = c

    def set_details(self, d):
        self.details = d


def _servicer(hub, **kw):
    base = dict(zone_names=["frame", "door", "bay"], presence_q=512, model_size=(16, 12), serve_events=True)
    base.update(kw)
    return S.SemanticSegmentationV2Servicer(hub, {1: "car", 3: "person"}, **base)


def _filled():
    hub = ResultHub(1, event_log=64)
    f = lambda lab, root: (lab << 24) | root
    events = [(_w0(0, 0, 1, 1), 7, f(3, 17), 100), (_w0(0, 1, 1, 1), 7, f(3, 17), 60),
              (_w0(1, 2, 2, 0), 4, f(1, 9), 12), (_w0(1, 0, 2, 1), 5, f(1, 30), 44)]
    hub.push_events(np.stack([_frame(4, events[:2]), _frame(4, events[2:])]), np.array([[20, 0, 1.5], [21, 0, 2.5]]))
    return hub


def test_servicer_status_codes_fields_filter_cursor_and_limit():
    hub = _filled()
    on, off = _servicer(hub), _servicer(hub, serve_events=False)
    ctx = _Ctx()
    off.GetZoneEvents(P.EventRequest(stream_id=0), ctx)
    assert ctx.code == grpc.StatusCode.FAILED_PRECONDITION and "--serve_events" in ctx.details
    ctx = _Ctx()
    on.GetZoneEvents(P.EventRequest(stream_id=5), ctx)
    assert ctx.code == grpc.StatusCode.NOT_FOUND
    ctx = _Ctx()
    m = on.GetZoneEvents(P.EventRequest(stream_id=0), ctx)
    assert ctx.code is None and (m.stream_id, m.next_seq, m.lost, m.truncated, m.min_share) == (0, 4, 0, 0, 0.5)
    assert [(e.seq, e.epoch, e.kind, e.frame_id, e.timestamp, e.zone, e.zone_name, e.track_id, e.class_id, e.label,
             e.root, e.track_edge, e.pixels, e.dwell) for e in m.events] == [
        (1, 0, 1, 20, 1.5, 0, "frame", 7, 3, "person", 17, True, 100, 0),
        (2, 0, 1, 20, 1.5, 1, "door", 7, 3, "person", 17, True, 60, 0),
        (3, 0, 2, 21, 2.5, 2, "bay", 4, 1, "car", 9, False, 0, 12),
        (4, 0, 2, 21, 2.5, 0, "frame", 5, 1, "car", 30, True, 0, 44)]
    # an empty answer is ordinary: no UNAVAILABLE, next_seq = after_seq
    ctx = _Ctx()
    m = on.GetZoneEvents(P.EventRequest(stream_id=0, after_seq=4), ctx)
    assert ctx.code is None and len(m.events) == 0 and m.next_seq == 4
    quiet = _servicer(ResultHub(1))
    ctx = _Ctx()
    m = quiet.GetZoneEvents(P.EventRequest(stream_id=0), ctx)
    assert ctx.code is None and len(m.events) == 0 and m.next_seq == 0
    # the cursor, max_events, and the zone filter after the cursor (gaps in seq)
    m = on.GetZoneEvents(P.EventRequest(stream_id=0, after_seq=1, max_events=2), _Ctx())
    assert [e.seq for e in m.events] == [2, 3] and m.next_seq == 3
    m = on.GetZoneEvents(P.EventRequest(stream_id=0, zones=[0]), _Ctx())
    assert [e.seq for e in m.events] == [1, 4] and m.next_seq == 4
    m = on.GetZoneEvents(P.EventRequest(stream_id=0, zones=[2, 1], max_events=3), _Ctx())
    assert [e.seq for e in m.events] == [2, 3] and m.next_seq == 3
    hub.bump_epoch([0])
    hub.push_events(_frame(1, [_ev(1)], n=6)[None], np.array([[30, 0, 3.0]]))
    m = on.GetZoneEvents(P.EventRequest(stream_id=0, after_seq=4), _Ctx())
    assert [(e.seq, e.epoch) for e in m.events] == [(5, 1)] and m.truncated == 5


def test_v2_has_the_rpc_and_the_readable_proto_lists_it():
    assert "GetZoneEvents" in P.V2_METHODS and "GetZoneEvents" not in P.V1_METHODS
    v2 = {m.name: {f.name: (f.number, f.type) for f in m.field} for m in P.v2_file_descriptor().message_type}
    F = P.F
    assert v2["EventRequest"] == {"stream_id": (1, F.TYPE_INT32), "after_seq": (2, F.TYPE_UINT64),
                                  "max_events": (3, F.TYPE_INT32), "zones": (4, F.TYPE_INT32)}
    assert v2["ZoneEvent"] == {
        "seq": (1, F.TYPE_UINT64), "epoch": (2, F.TYPE_UINT32), "kind": (3, F.TYPE_INT32),
        "frame_id": (4, F.TYPE_INT64), "timestamp": (5, F.TYPE_DOUBLE), "zone": (6, F.TYPE_INT32),
        "zone_name": (7, F.TYPE_STRING), "track_id": (8, F.TYPE_UINT32), "class_id": (9, F.TYPE_INT32),
        "label": (10, F.TYPE_STRING), "root": (11, F.TYPE_UINT32), "track_edge": (12, F.TYPE_BOOL),
        "pixels": (13, F.TYPE_UINT32), "dwell": (14, F.TYPE_UINT32)}
    assert v2["ZoneEvents"] == {"stream_id": (1, F.TYPE_INT32), "events": (2, F.TYPE_MESSAGE),
                                "next_seq": (3, F.TYPE_UINT64), "lost": (4, F.TYPE_UINT64),
                                "truncated": (5, F.TYPE_UINT64), "min_share": (6, F.TYPE_FLOAT)}
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                        "semantic_segmentation_server_amd", "api", "sem_seg_server_v2.proto")
    with open(path) as f:
        text = f.read()
    assert "rpc GetZoneEvents(EventRequest) returns (ZoneEvents)" in text
    for name in ("EventRequest", "ZoneEvent", "ZoneEvents"):
        assert f"message {name} " in text
        for fname, (num, _) in v2[name].items():
            assert f" {fname} = {num};" in text, (name, fname)


# ---- config --------------------------------------------------------------------------------------

ON = ["--serve_regions", "--serve_zones", "--serve_presence", "--track_regions", "--serve_events"]


def test_cli_flags_and_every_refusal():
    d = C.parse([])
    assert (d.serve_events, d.max_events, d.event_log) == (False, 64, 4096)
    cfg = C.parse(ON + ["--max_events", "16", "--event_log", "32"])
    assert cfg.serve_events and (cfg.max_events, cfg.event_log) == (16, 32)
    for argv in (["--serve_events"], ["--serve_regions", "--serve_zones", "--serve_presence", "--serve_events"],
                 ["--serve_regions", "--track_regions", "--serve_events"]):
        with pytest.raises(ValueError) as e:
            C.parse(argv)
        assert "--serve_events" in str(e.value) and "--serve_presence" in str(e.value) \
            and "--track_regions" in str(e.value)
    with pytest.raises(ValueError, match="--serve_regions"):     # refused where its parents are
        C.parse(["--serve_zones", "--serve_presence", "--track_regions", "--serve_events"])
    for E in ("0", "4097"):
        with pytest.raises(ValueError, match="--max_events"):
            C.parse(ON + ["--max_events", E])
    with pytest.raises(ValueError, match="--event_log"):
        C.parse(ON + ["--max_events", "64", "--event_log", "63"])
    C.parse(ON + ["--max_events", "64", "--event_log", "64"])


# ---- engine, server and client on the CPU --------------------------------------------------------

@pytest.fixture(scope="module")
def zone_file(tmp_path_factory):
    p = tmp_path_factory.mktemp("events") / "zones.json"
    p.write_text(json.dumps(PC.ZONES))
    return str(p)


def _cfg(**kw):
    base = dict(backend="torch", device="cpu", input_size=65, batch=1, port=0, host="127.0.0.1",
                min_area_ratio=0.0005, fps_limit=200.0, log_level="WARNING")
    base.update(kw)
    return C.Config(**base)


def _on(zone_file, **kw):
    return _cfg(serve_regions=True, serve_zones=True, zones=zone_file, serve_presence=True, track_regions=True,
                serve_events=True, **kw)


def test_engine_step_events_on_cpu(zone_file):
    from semantic_segmentation_server_amd.runtime.engine import Engine
    from semantic_segmentation_server_amd.runtime.sources import SyntheticSource
    eng = Engine(_on(zone_file, batch=2, streams=2, max_regions=8, max_events=16))
    assert eng.event_cap == 16
    src = SyntheticSource(160, 120, pool=4, seed=3)
    prev = [None, None]
    total = 0
    for step in range(3):
        f, _, _ = src.read_batch(2)
        eng.step(f, [step, step], [0.0, 0.0], [0, 1])
        assert eng.events.shape == (2, 4 + 4 * 16) and eng.events.dtype == np.uint32
        for b in range(2):
            want = EV.events_between(prev[b], eng.presence[b], 4, 16)
            assert np.array_equal(eng.events[b], want), (step, b)
            prev[b] = eng.presence[b].copy()
            total += int(want[0])
            if step == 0:   # every stored region is born
                assert int(want[0]) >= int(eng.presence[b][0])
    assert total > 0
    eng.reset_tracks()                     # forgets the previous rows with the tracks
    f, _, _ = src.read_batch(2)
    eng.step(f, [9, 9], [0.0, 0.0], [0, 1])
    for b in range(2):
        assert np.array_equal(eng.events[b], EV.events_between(None, eng.presence[b], 4, 16))
    # flag off: nothing else changes
    off = Engine(_cfg(serve_regions=True, serve_zones=True, zones=zone_file, serve_presence=True,
                      track_regions=True, batch=2, streams=2, max_regions=8))
    on2 = Engine(_on(zone_file, batch=2, streams=2, max_regions=8))
    f, _, _ = SyntheticSource(160, 120, pool=4, seed=3).read_batch(2)
    r_on, r_off = on2.step(f, [0, 0], [0.0, 0.0], [0, 1]), off.step(f, [0, 0], [0.0, 0.0], [0, 1])
    assert off.events is None and off.event_cap == 0 and off._events is None and r_on.tobytes() == r_off.tobytes()
    assert np.array_equal(on2.presence, off.presence) and np.array_equal(on2.regions, off.regions)


def test_engine_refuses_the_flag_without_its_parents(zone_file):
    from semantic_segmentation_server_amd.runtime.engine import Engine
    for name in ("serve_presence", "track_regions"):
        bad = _on(zone_file).replace()
        object.__setattr__(bad, name, False)
        with pytest.raises(ValueError, match="--serve_events"):
            Engine(bad)


@pytest.mark.parametrize("serve", [True, False])
def test_server_and_client_on_cpu(serve, zone_file, capsys):
    """Batches of two frames of one stream: the log holds the events of BOTH frames of a step."""
    from semantic_segmentation_server_amd import client
    from semantic_segmentation_server_amd.server import Server
    cfg = _on(zone_file, fps_limit=None, batch=2, max_regions=8) if serve else \
        _cfg(serve_regions=True, serve_zones=True, zones=zone_file, serve_presence=True, track_regions=True,
             fps_limit=None, batch=2, max_regions=8)
    srv = Server(cfg, max_steps=3).start()
    try:
        srv.producer.join(timeout=120)
        assert srv.producer.steps == 3 and srv.producer.error is None
        target = f"127.0.0.1:{srv.port}"
        if not serve:
            with grpc.insecure_channel(target) as ch:
                with pytest.raises(grpc.RpcError) as e:
                    S.SemanticSegmentationV2Stub(ch).GetZoneEvents(P.EventRequest(stream_id=0))
            assert e.value.code() == grpc.StatusCode.FAILED_PRECONDITION
            assert client.main(["--target", target, "--events"]) == 1
            assert len(srv.hub.events_after(0, 0)[0]) == 0
            return
        m = client.fetch_events(target, 0)
        assert len(m.events) > 0 and [e.seq for e in m.events] == list(range(1, len(m.events) + 1))
        assert m.next_seq == len(m.events) and m.lost == 0 and m.min_share == 0.5
        fids = [e.frame_id for e in m.events]
        assert fids == sorted(fids) and fids[0] == 0 and set(fids) <= set(range(6))
        first = [e for e in m.events if e.frame_id == 0]
        assert all(e.kind == 1 and e.track_edge for e in first if e.zone == 0) and any(e.zone == 0 for e in first)
        # frames that are not the last of their step are in the log whenever they have events
        ev, _, _ = srv.hub.events_after(0, 0, 4096)
        assert len(ev) == len(m.events)
        again = client.fetch_events(target, 0, after_seq=m.next_seq)
        assert len(again.events) == 0 and again.next_seq == m.next_seq
        capsys.readouterr()
        assert client.main(["--target", target, "--events", "0"]) == 0
        text = capsys.readouterr().out
        assert len(text.strip().splitlines()) == len(m.events) and "ENTER" in text and "(track begins)" in text
        e = m.events[0]
        assert f"track {e.track_id:>5}" in text and e.zone_name in text
    finally:
        srv.stop(0)


def test_pipeline_on_cpu_pushes_every_frame(zone_file):
    from semantic_segmentation_server_amd.parallel.dist import DistContext
    from semantic_segmentation_server_amd.parallel.dp import DataParallelPipeline
    from semantic_segmentation_server_amd.runtime.engine import Engine
    from semantic_segmentation_server_amd.runtime.sources import SyntheticSource
    eng = Engine(_on(zone_file, batch=2, max_regions=8, max_events=32))
    hub = ResultHub(1)
    pipe = DataParallelPipeline(DistContext(), eng, 160, 120, 2, "local", hub, lag=1)
    src = SyntheticSource(160, 120, pool=6, seed=5)
    batches = [torch.from_numpy(src.read_batch(2)[0].copy()) for _ in range(3)]
    pipe.prefetch(batches[0])
    for k in range(3):
        pipe.step(frame_ids=[2 * k, 2 * k + 1], ts=[k + 0.0, k + 0.5], streams=[0, 0],
                  next_frames=batches[k + 1] if k < 2 else None)
    pipe.flush()
    ev, nxt, lost = hub.events_after(0, 0, 4096)
    # the oracle: the engine's definition over the same label maps, one stream, frame after frame
    ref = Engine(_on(zone_file, batch=2, max_regions=8, max_events=32))
    want = []
    for k, f in enumerate(batches):
        ref.step(f.numpy(), [2 * k, 2 * k + 1], [k + 0.0, k + 0.5], [0, 0])
        for b in range(2):
            d = ref.events[b]
            for j in range(min(int(d[0]), 32)):
                want.append((2 * k + b, k + 0.5 * b) + tuple(int(v) for v in d[4 + 4 * j:8 + 4 * j]))
    got = [(int(e["frame_id"]), float(e["ts"]), int(e["w0"]), int(e["w1"]), int(e["w2"]), int(e["w3"])) for e in ev]
    assert got == want and len(want) > 0 and nxt == len(want) and lost == 0
    assert len({w[0] for w in want}) > 1


def test_supervised_server_on_cpu(zone_file):
    """The fifth channel end to end: a worker process pushes its events into the ring, the parent's
    hub numbers them, the RPC serves them."""
    import time
    from semantic_segmentation_server_amd.runtime.supervisor import SupervisedServer
    sup = SupervisedServer(_on(zone_file, max_regions=8), heartbeat_timeout_s=60.0).start()
    try:
        t_end = time.time() + 240
        while sup.hub.events_after(0, 0, 1)[1] == 0 and time.time() < t_end and sup.alive:
            time.sleep(0.05)
        ev, nxt, lost = sup.hub.events_after(0, 0, 4096)
        assert len(ev) > 0, sup.error
        assert ev["seq"].tolist() == list(range(1, len(ev) + 1)) and (ev["epoch"] == 0).all() and lost == 0
        assert (np.diff(ev["frame_id"]) >= 0).all() and (ev["stream"] == 0).all()
        d = EV.decode(np.stack([ev["w0"], ev["w1"], ev["w2"], ev["w3"]], 1))
        first = d[ev["frame_id"] == ev["frame_id"][0]]
        assert (first["kind"] == EV.ENTER).all() and (first["zone"] == 0).any()   # the first frame: births
        with grpc.insecure_channel(f"127.0.0.1:{sup.port}") as ch:
            m = S.SemanticSegmentationV2Stub(ch).GetZoneEvents(P.EventRequest(stream_id=0, max_events=len(ev)))
        assert [e.seq for e in m.events] == ev["seq"].tolist() and m.next_seq == len(ev)
        assert [e.track_id for e in m.events] == d["track_id"].tolist() and m.min_share == 0.5
    finally:
        sup.stop(0)
