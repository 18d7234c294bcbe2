"""Device zone events (csrc/hip/zone_events.hip) against the numpy definition
(postprocess/events.py), and the engine / pipeline layers that carry its output.

Every comparison is exact on the uint32 words, and on the whole row: ``out`` is prefilled with a
sentinel (every word must be written) and the state is over-allocated by a sentinel tail that must
come back unchanged. The kernel cases run on presence rows built by hand (tests/event_cases.py):
the kernels read nothing else. The chain cases run ``class_regions``, ``region_tracks`` and
``zone_presence`` first (the buffers of tests/test_presence_gpu.py).
"""
import numpy as np
import pytest
import torch

import event_cases as EC
import presence_cases as PC
import test_presence_gpu as TP
from semantic_segmentation_server_amd.postprocess import events as EV
from semantic_segmentation_server_amd.postprocess import presence as PR

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENT = EC.SENT
ST_SENT = 0xA5
ST_TAIL = 256
BIG = 0xFFFFFFFF


def _hip():
    from semantic_segmentation_server_amd.ops import hip_ops
    return hip_ops


class _Kernel:
    """zone_events on static buffers for one batch layout. ``state``: a shared buffer of
    ``state_bytes + ST_TAIL`` bytes (default: its own, zero with a sentinel tail)."""

    def __init__(self, counts, K, R, E, state=None):
        hip = _hip()
        self.counts, self.K, self.R, self.E = list(counts), K, R, E
        self.B = sum(counts)
        self.rows = torch.zeros((self.B, PR.frame_words(K, R, True)), dtype=torch.int32, device=DEV)
        self.out = torch.full((self.B, EV.frame_words(E)), SENT, dtype=torch.int32, device=DEV)
        self.nb = hip.zone_events_state_bytes(len(counts), K, R)
        assert self.nb == len(counts) * 4 * PR.frame_words(K, R, True)
        if state is None:
            state = torch.full((self.nb + ST_TAIL,), ST_SENT, dtype=torch.uint8, device=DEV)
            state[:self.nb] = 0
        self.buf = state
        self.state = state[:self.nb]
        self.tables = hip.region_track_tables(counts, DEV)

    def launch(self):
        _hip().zone_events(self.rows, self.out, self.state, self.tables, counts=self.counts, K=self.K,
                           R=self.R, E=self.E)

    def load(self, rows):
        self.rows.copy_(torch.from_numpy(np.ascontiguousarray(np.stack(rows)).view(np.int32)))

    def step(self, rows):
        """One batch (its B presence rows in row order) -> the event rows, uint32."""
        self.load(rows)
        self.out.fill_(SENT)
        self.launch()
        torch.cuda.synchronize()
        assert (self.buf[self.nb:].cpu().numpy() == ST_SENT).all()
        return self.out.cpu().numpy().view(np.uint32)


def _same_rows(got, want, what=""):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(got[:4], want[:4]), (what, got[:4], want[:4])
    assert np.array_equal(got, want), (what, np.flatnonzero(got != want)[:8])


def _run(seqs, counts, K, R, E, kernel=None):
    """Feed the streams' row sequences through a kernel of this layout until one runs out -> per
    stream the list of its event rows."""
    kern = kernel or _Kernel(counts, K, R, E)
    pos = [0] * len(seqs)
    got = [[] for _ in seqs]
    while all(pos[s] + c <= len(seqs[s]) for s, c in enumerate(counts)):
        rows, owner = [], []
        for s, c in enumerate(counts):
            rows += seqs[s][pos[s]:pos[s] + c]
            owner += [s] * c
            pos[s] += c
        for ev, s in zip(kern.step(rows), owner):
            got[s].append(ev.copy())
    return got


def _same(got, want):
    assert len(got) == len(want) > 0
    for k, (g, w) in enumerate(zip(got, want)):
        _same_rows(g, w, k)


def _pair(prev, cur, K, R, E):
    """prev then cur as one stream's batch of two, and as two steps of one: both equal the oracle."""
    want = EC.oracle([prev, cur], R, E)
    _same(_run([[prev, cur]], [2], K, R, E)[0], want)
    _same(_run([[prev, cur]], [1], K, R, E)[0], want)
    return want


# ---- kernel on built rows --------------------------------------------------------------------------

def test_one_entry_one_row():
    K = R = 1
    seq = [EC.row(K, R, [1], [[1]]), EC.row(K, R, [1], [[2]]), EC.row(K, R, [], np.zeros((0, 1))),
           EC.row(K, R, [2], [[1]]), EC.row(K, R, [3], [[BIG]]), EC.row(K, R, [3], [[0]])]
    want = EC.oracle(seq, R, 4)
    assert [int(w[0]) for w in want] == [1, 0, 1, 1, 1, 1]
    _same(_run([seq], [1], K, R, 4)[0], want)
    _same(_run([seq], [3], K, R, 1)[0], EC.oracle(seq, R, 1))


@pytest.mark.parametrize("E", [4096, 1])
def test_every_entry_of_256_flips_in_33_rows(E):
    prev, cur = EC.all_flip(256, 33)
    want = _pair(prev, cur, 256, 33, E)
    assert int(want[1][0]) == 2 * 8448 and int(want[0][0]) == 0
    d = EV.decode(want[1])
    assert len(d) == E and (d["kind"] == 2).all()
    # and with room for none of the ENTERs but the count of all: prev -> cur -> prev
    got = _run([[prev, cur, prev]], [3], 256, 33, E)[0]
    _same(got, EC.oracle([prev, cur, prev], 33, E))


@pytest.mark.parametrize("total", [7, 8, 9])
def test_totals_around_the_capacity(total):
    K, R, E, pn, cn = 12, 6, 8, 11, 9
    cand = [0, 7, 20, 41, 65, 66, 80, 100, 119][:total]
    prev, cur = EC.events_at(K, R, pn, cn, cand)
    want = _pair(prev, cur, K, R, E)
    assert int(want[1][0]) == total and EV.used_words(want[1]) == 4 + 4 * min(total, E)


@pytest.mark.parametrize("shape", [(256, 33, 200, 256), (256, 33, 256, 2), (12, 6, 11, 9), (64, 4, 64, 64),
                                   (64, 2, 64, 64)])
def test_events_only_at_the_scan_boundaries(shape):
    """Candidates 0, 63, 64, 255, 256, the last LEAVE, the first ENTER and the last candidate: the
    lane, wave and LEAVE / ENTER boundaries of the compaction."""
    K, R, pn, cn = shape
    cand = EC.boundary_candidates(pn, cn, R)
    prev, cur = EC.events_at(K, R, pn, cn, cand)
    want = _pair(prev, cur, K, R, 64)
    d = EV.decode(want[1])
    assert [int(e["slot"]) * R + int(e["zone"]) + (pn * R if e["kind"] == 1 else 0) for e in d] == cand
    for c in cand:   # and each boundary alone
        p1, c1 = EC.events_at(K, R, pn, cn, [c])
        got = _run([[p1, c1]], [2], K, R, 2)[0]
        _same(got, EC.oracle([p1, c1], R, 2))
        assert int(got[1][0]) == 1


def test_empty_frames_and_the_largest_dwell():
    K, R = 5, 3
    none = EC.row(K, R, [], np.zeros((0, R)))
    a = EC.row(K, R, [1, 2, 3], [[BIG, BIG, 0], [1, 0, BIG], [BIG, 1, 1]])
    b = EC.row(K, R, [3, 1, 4], [[BIG, 0, 2], [0, BIG, BIG], [1, BIG, 0]])
    seq = [none, a, b, none, none, b, a]
    want = EC.oracle(seq, R, 16)
    assert int(want[0][0]) == 0 and int(want[4][0]) == 0 and BIG in want[2][4:].tolist()
    for counts in ([1], [7], [2]):
        _same(_run([seq], counts, K, R, 16)[0], want[:len(seq) // counts[0] * counts[0]])


def test_seeded_random_cases():
    """200 tiny cases: random K, R, E and batch layout over random row sequences."""
    rng = np.random.default_rng(2025)
    events = 0
    for case in range(200):
        K, R = int(rng.integers(1, 13)), int(rng.integers(1, 7))
        B, E = int(rng.integers(1, 5)), int(rng.integers(1, 9))
        S = int(rng.integers(1, min(B, 2) + 1))
        counts = [B] if S == 1 else [B - B // 2, B // 2]
        seqs = [EC.random_sequence(rng, K, R, 2 * c) for c in counts]
        got = _run(seqs, counts, K, R, E)
        for s in range(S):
            want = EC.oracle(seqs[s], R, E)
            _same(got[s], want)
            events += sum(int(w[0]) for w in want)
    assert events > 2000


# ---- batch layouts and state -----------------------------------------------------------------------

LK, LR, LE = 6, 4, 8


def _layout_seqs():
    rng = np.random.default_rng(77)
    return EC.random_sequence(rng, LK, LR, 8), EC.random_sequence(rng, LK, LR, 4)


def test_every_batching_gives_the_same_event_rows():
    s0, s1 = _layout_seqs()
    w0, w1 = EC.oracle(s0, LR, LE), EC.oracle(s1, LR, LE)
    assert sum(int(w[0]) for w in w0) > 8 and max(int(w[0]) for w in w0) > LE   # truncation occurs
    _same(_run([s0], [1], LK, LR, LE)[0], w0)
    _same(_run([s0], [4], LK, LR, LE)[0], w0)
    a, b = _run([s0, s1], [2, 2], LK, LR, LE)
    _same(a, w0[:4])
    _same(b, w1)
    a, b = _run([s0, s1], [2, 1], LK, LR, LE)
    _same(a, w0)
    _same(b, w1)
    a, b = _run([s0, s1], [1, 0], LK, LR, LE)
    _same(a, w0)
    assert b == []


def test_a_stream_without_a_row_keeps_its_state_and_zero_is_a_reset():
    s0, s1 = _layout_seqs()
    w0, w1 = EC.oracle(s0, LR, LE), EC.oracle(s1, LR, LE)
    both = _Kernel([1, 1], LK, LR, LE)
    only0 = _Kernel([1, 0], LK, LR, LE, state=both.buf)   # stream 1 has no row
    got0, got1 = [], []
    r = both.step([s0[0], s1[0]])
    got0.append(r[0].copy()), got1.append(r[1].copy())
    before = both.state.cpu().numpy().view(np.uint32).reshape(2, -1)[1].copy()
    got0.append(only0.step([s0[1]])[0].copy())
    got0.append(only0.step([s0[2]])[0].copy())
    assert np.array_equal(both.state.cpu().numpy().view(np.uint32).reshape(2, -1)[1], before)
    r = both.step([s0[3], s1[1]])
    got0.append(r[0].copy()), got1.append(r[1].copy())
    _same(got0, w0[:4])
    _same(got1, w1[:2])
    # the state of a stream is the used words of its last presence row
    st = both.state.cpu().numpy().view(np.uint32).reshape(2, -1)
    for s, last in ((0, s0[3]), (1, s1[1])):
        u = PR.used_words(last, LR, True)
        assert np.array_equal(st[s][:u], last[:u])
    both.state.zero_()                                    # a reset: every current track ENTERs
    r = both.step([s0[4], s1[2]])
    for g, cur in zip(r, (s0[4], s1[2])):
        _same_rows(g, EV.events_between(None, cur, LR, LE))
        p = PR.decode(cur, LR, True)
        assert int(g[0]) == int((p.D == 1).sum())


# ---- the full chain --------------------------------------------------------------------------------

class _Full:
    """The chain of tests/test_presence_gpu.py with zone_events at its end."""

    def __init__(self, counts, E=16):
        self.chain = TP._seq_chain(counts)
        self.ev = _Kernel(counts, PC.SK, 4, E)
        self.ev.tables = self.chain.tables

    def launch(self):
        c, e = self.chain, self.ev
        c.launch()
        _hip().zone_events(c.out, e.out, e.state, c.tables, counts=c.counts, K=c.K, R=c.R, E=e.E)

    def step(self, maps):
        self.chain.load(maps)
        self.chain.out.fill_(TP.SENT)
        self.ev.out.fill_(SENT)
        self.launch()
        torch.cuda.synchronize()
        assert (self.ev.buf[self.ev.nb:].cpu().numpy() == ST_SENT).all()
        return self.ev.out.cpu().numpy().view(np.uint32)


def _run_full(seqs, counts):
    full = _Full(counts)
    pos = [0] * len(seqs)
    got = [[] for _ in seqs]
    while all(pos[s] + c <= len(seqs[s]) for s, c in enumerate(counts)):
        maps, owner = [], []
        for s, c in enumerate(counts):
            maps += seqs[s][pos[s]:pos[s] + c]
            owner += [s] * c
            pos[s] += c
        for ev, s in zip(full.step(maps), owner):
            got[s].append(ev.copy())
    return got


def _seq_wants(E=16):
    o0, o1 = PC.sequence_oracles()
    return EC.oracle([p for _, p in o0], 4, E), EC.oracle([p for _, p in o1], 4, E)


def test_full_chain_equals_the_cpu_words_in_every_batching():
    s0, s1 = (list(s) for s in PC.sequences())
    w0, w1 = _seq_wants()
    assert sum(int(w[0]) for w in w0) >= 8
    _same(_run_full([s0], [1])[0], w0)
    _same(_run_full([s0], [4])[0], w0)
    a, b = _run_full([s0, s1], [2, 2])
    _same(a, w0[:4])
    _same(b, w1)
    a, b = _run_full([s0, s1], [2, 1])
    _same(a, w0)
    _same(b, w1)
    _same(_run_full([s1], [3])[0], w1[:3])


def test_graph_replay_on_new_contents_keeps_the_state():
    s0, _ = PC.sequences()
    w0, _ = _seq_wants()
    full = _Full([2])
    full.chain.load(s0[0:2])
    full.launch()                          # warm-up outside capture; it advances the state:
    torch.cuda.synchronize()
    full.chain.state.zero_()
    full.chain.pstate.zero_()
    full.ev.state.zero_()                  # reset before the captured runs
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g):
            full.launch()
    torch.cuda.current_stream().wait_stream(s)
    got = []
    for k in range(4):
        full.chain.load(s0[2 * k:2 * k + 2])
        full.ev.out.fill_(SENT)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        ev = full.ev.out.cpu().numpy().view(np.uint32)
        got += [ev[0].copy(), ev[1].copy()]
    _same(got, w0)
    assert (full.ev.buf[full.ev.nb:].cpu().numpy() == ST_SENT).all()


# ---- copy kernel and wrapper -----------------------------------------------------------------------

@pytest.mark.parametrize("E", [1, 8, 4096])
def test_copy_to_host_moves_exactly_the_used_words(E):
    hip = _hip()
    rng = np.random.default_rng(E)
    B = 5
    src = rng.integers(1, 1 << 32, (B, EV.frame_words(E)), dtype=np.uint64).astype(np.uint32)
    src[:, 0] = [0, 1, E, E + 1, max(1, E // 2)]
    dev = torch.from_numpy(src.view(np.int32)).to(DEV)
    dst = torch.full((B, EV.frame_words(E)), SENT, dtype=torch.int32).pin_memory()
    hip.zone_events_copy_to_host(dev, dst, E)
    torch.cuda.synchronize()
    got = dst.numpy().view(np.uint32)
    for b in range(B):
        u = EV.used_words(src[b])
        assert np.array_equal(got[b, :u], src[b, :u]) and (got[b, u:] == SENT).all(), b
    for bad in (dict(src=dev.cpu()), dict(dst=torch.zeros_like(dst)), dict(E=E + 1), dict(src=dev[:, :-1]),
                dict(dst=dst[:-1])):
        a = dict(src=dev, dst=dst, E=E)
        a.update(bad)
        with pytest.raises(ValueError):
            hip.zone_events_copy_to_host(a["src"], a["dst"], a["E"])


def test_wrapper_rejects_bad_arguments_without_launching():
    hip = _hip()
    K, R, E = 4, 3, 5
    k = _Kernel([1, 1], K, R, E)
    k.load([EC.row(K, R, [1, 2], [[1, 1, 1], [1, 0, 1]])] * 2)
    k.state.fill_(ST_SENT)
    one = _Kernel([2], K, R, E)

    def go(exc, **kw):
        a = dict(presence_rows=k.rows, out=k.out, state=k.state, tables=k.tables, counts=[1, 1], K=K, R=R, E=E)
        a.update(kw)
        pos = [a.pop(n) for n in ("presence_rows", "out", "state", "tables")]
        with pytest.raises(exc):
            hip.zone_events(*pos, **a)

    go(ValueError, presence_rows=k.rows.cpu())
    go(TypeError, presence_rows=k.rows.float())
    go(ValueError, presence_rows=k.rows[:1])
    go(ValueError, presence_rows=k.rows[:, :-1])
    wide = torch.full((2, 2 * k.rows.shape[1]), SENT, dtype=torch.int32, device=DEV)
    go(ValueError, presence_rows=wide[:, ::2])                 # not contiguous
    go(TypeError, out=k.out.float())
    go(ValueError, out=k.out[:, :-4])
    go(ValueError, out=k.out.cpu())
    go(ValueError, out=k.rows, E=8)                            # out is presence_rows (4 + 8 K words both)
    go(ValueError, K=0)
    go(ValueError, K=257)
    go(ValueError, R=0)
    go(ValueError, R=34)
    go(ValueError, E=0)
    go(ValueError, E=4097)
    go(ValueError, E=E + 1)
    go(ValueError, K=K + 1)
    go(ValueError, R=R + 1)
    go(ValueError, counts=[2])                                 # state and tables are for two streams
    go(ValueError, counts=[1, 2])
    go(ValueError, counts=[1, -1])
    go(ValueError, counts=[])
    go(ValueError, counts=[2, 0], tables=one.tables)
    go(ValueError, state=k.buf[:k.nb - 4])
    go(ValueError, state=k.buf[:k.nb + 4])                     # an exact size
    go(TypeError, state=k.state.view(torch.int32))
    go(ValueError, state=k.state.cpu())
    go(ValueError, tables=k.tables[:-1])
    go(TypeError, tables=k.tables.float())
    go(ValueError, tables=k.tables.cpu())
    torch.cuda.synchronize()
    assert (k.out.cpu().numpy() == SENT).all() and (k.buf.cpu().numpy() == ST_SENT).all()
    assert (wide.cpu().numpy() == SENT).all()
    with pytest.raises(RuntimeError):                          # the launcher itself checks its arguments
        hip._hip_mod().zone_events(k.rows.data_ptr(), k.out.data_ptr(), 0, k.tables.data_ptr(),
                                   k.tables.data_ptr() + 8, k.tables.data_ptr() + 16, 2, 2, K, R, E, 0)
    torch.cuda.synchronize()
    assert (k.out.cpu().numpy() == SENT).all()


# ---- engine and pipeline ---------------------------------------------------------------------------

zone_file = TP.zone_file


def _on(zone_file, **kw):
    return TP._on(zone_file, track_regions=True, streams=2, serve_events=True, **kw)


@pytest.mark.parametrize("graph", [False, True])
def test_engine_step_events_are_those_of_its_labels(graph, zone_file):
    from semantic_segmentation_server_amd.runtime.engine import Engine
    from semantic_segmentation_server_amd.runtime.sources import SyntheticSource
    eng = Engine(_on(zone_file, graph=graph), torch.device(DEV))
    assert eng.event_cap == 64
    src = SyntheticSource(200, 150, pool=6, seed=7)
    first, _, _ = src.read_batch(2)
    eng.step(first, [0, 1], [1.0, 2.0], [0, 1])   # builds (and with graph captures) the step:
    eng.reset_tracks()                            # warm-up and capture advance the state
    orc = TP._Oracle(eng)
    prev = [None, None]
    seen = 0
    for k in range(3):
        f, _, _ = src.read_batch(2)
        eng.step(f, [2 * k, 2 * k + 1], [1.0, 2.0], [0, 1])
        got = eng.events.copy()
        assert got.shape == (2, 4 + 4 * 64) and got.dtype == np.uint32
        want = orc.rows(torch.from_numpy(f))
        for b in range(2):
            _same_rows(eng.presence[b], want[b], (k, b))
            _same_rows(got[b], EV.events_between(prev[b], want[b], 4, 64), (k, b))
            prev[b] = want[b]
            seen += int(got[b][0])
    assert seen > 0


def _oracle_log(eng, batches, n_streams=2):
    """Per stream [(frame_id, ts, w0, w1, w2, w3)] of the events of ``batches`` as TP._drive feeds
    them, by the definition over the engine's own label maps."""
    orc = TP._Oracle(eng)
    prev = [None] * n_streams
    want = [[] for _ in range(n_streams)]
    for k, f in enumerate(batches):
        rows = orc.rows(f)
        for s in range(n_streams):
            ev = EV.events_between(prev[s], rows[s], 4, eng.event_cap)
            prev[s] = rows[s]
            for j in range((EV.used_words(ev) - 4) // 4):
                want[s].append((100 + 2 * k + s, 1.0 + k + 0.5 * s) + tuple(int(v) for v in ev[4 + 4 * j:8 + 4 * j]))
    return want


def test_pipeline_logs_every_frame_and_flag_off_is_the_parent(zone_file):
    from semantic_segmentation_server_amd.runtime.engine import Engine
    from semantic_segmentation_server_amd.runtime.results import ResultHub
    n = 2 * 3 + 1  # 2 * nslots + 1
    batches = TP._batches(n)
    eng = Engine(_on(zone_file, graph=True), torch.device(DEV))
    hub = ResultHub(2, maxlen=100000)
    pipe, recs = TP._drive(eng, batches, hub)
    assert pipe.local_events is not None and len(pipe.local_events) == pipe.nslots
    want = _oracle_log(eng, batches)
    for s in range(2):
        ev, nxt, lost = hub.events_after(s, 0, 4096)
        got = [(int(e["frame_id"]), float(e["ts"]), int(e["w0"]), int(e["w1"]), int(e["w2"]), int(e["w3"])) for e in ev]
        assert got == want[s] and len(got) > 0 and (nxt, lost) == (len(got), 0)
        assert ev["seq"].tolist() == list(range(1, len(got) + 1)) and hub.events_truncated(s) == 0
        assert len({g[0] for g in got}) > 1      # more frames than the last one
    pre_on = [hub.presence(s).words.copy() for s in range(2)]
    reg_on = [hub.regions(s).words.copy() for s in range(2)]
    zon_on = [hub.zones(s).words.copy() for s in range(2)]
    # flag off: no launch, no buffer, and records, regions, zones and presence are bit-equal
    off = Engine(TP._on(zone_file, graph=True, track_regions=True, streams=2), torch.device(DEV))
    hub_off = ResultHub(2, maxlen=100000)
    pipe_off, recs_off = TP._drive(off, batches, hub_off)
    assert off.event_cap == 0 and off.events_packed is None and off.events is None and off._events is None
    assert pipe_off.local_events is None and pipe_off.event_cap == 0 and len(hub_off.events_after(0, 0)[0]) == 0
    post = off._hip_post
    assert post.event_cap == 0 and not post._event_bufs and not post._event_state and post.last_events is None
    assert len(recs) > 0 and recs.tobytes() == recs_off.tobytes()
    for s in range(2):
        assert np.array_equal(hub_off.regions(s).words, reg_on[s]) and np.array_equal(hub_off.zones(s).words, zon_on[s])
        assert np.array_equal(hub_off.presence(s).words, pre_on[s])
