"""Device region tracks (the k_tr_* kernels of csrc/hip/class_regions.hip) against the numpy
definition (postprocess/tracks.py), and the engine / pipeline layers that carry the wider rows.

Every comparison is exact on the uint32 words. The rows with tracks are prefilled with a
sentinel: words past the written range come back unchanged. Small shapes: a 48 x 80 map with a
45 x 70 crop (2 x 3 tiles of 32 x 32, ragged on both edges; pitch != width).
"""
import functools

import numpy as np
import pytest
import torch

from semantic_segmentation_server_amd.postprocess import regions as RG
from semantic_segmentation_server_amd.postprocess import tracks as TK

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENT = 0x5A5A5A5A
H, W, CH, CW = 48, 80, 45, 70
CLS = [1, 2, 3, 4, 5]
KS = 6  # records of the sequence tests: fewer than the regions of any of their frames


def _hip():
    from semantic_segmentation_server_amd.ops import hip_ops
    return hip_ops


class _Chain:
    """class_regions + region_tracks on static buffers for one batch layout."""

    def __init__(self, counts, K, min_pixels, classes=CLS, geom=(H, W, CH, CW), q=256, state=None):
        hip = _hip()
        self.counts, self.K, self.mp, self.classes, self.q = list(counts), K, min_pixels, classes, q
        self.H, self.W, self.ch, self.cw = geom
        B = self.B = sum(counts)
        self.lab = torch.zeros((B, self.H, self.W), dtype=torch.uint8, device=DEV)
        self.rows = torch.full((B, 4 + 6 * K), SENT, dtype=torch.int32, device=DEV)
        self.out = torch.full((B, 4 + 8 * K), SENT, dtype=torch.int32, device=DEV)
        self.ws = torch.zeros(hip.class_regions_workspace_bytes(B, self.ch, self.cw), dtype=torch.uint8, device=DEV)
        self.tws = torch.zeros(hip.region_tracks_workspace_bytes(B, self.ch, self.cw, K), dtype=torch.uint8,
                               device=DEV)
        self.state = state if state is not None else torch.zeros(
            hip.region_tracks_state_bytes(len(counts), self.ch, self.cw), dtype=torch.uint8, device=DEV)
        self.tables = hip.region_track_tables(counts, DEV)

    def launch(self):
        hip = _hip()
        hip.class_regions(self.lab, self.rows, self.ws, B=self.B, H=self.H, W=self.W, crop_h=self.ch,
                          crop_w=self.cw, classes=self.classes, min_pixels=self.mp, K=self.K)
        hip.region_tracks(self.rows, self.out, self.ws, self.tws, self.state, self.tables, counts=self.counts,
                          crop_h=self.ch, crop_w=self.cw, K=self.K, q=self.q)

    def step(self, maps):
        """One batch (its B maps in row order) -> uint32 [B, 4 + 8 K]."""
        self.lab.copy_(torch.from_numpy(np.ascontiguousarray(np.stack(maps), np.uint8)))
        self.out.fill_(SENT)
        self.launch()
        torch.cuda.synchronize()
        return self.out.cpu().numpy().view(np.uint32)


def _oracle(seq, K, min_pixels, classes=CLS, geom=(H, W, CH, CW), q=256):
    """The rows of one stream's sequence of maps by the definition."""
    tr = TK.StreamTracker(q)
    return [RG.encode(m, geom[3], geom[2], classes, min_pixels, K, out=np.full(4 + 8 * K, SENT, np.uint32),
                      tracker=tr) for m in seq]


def _run(seqs, counts, K, min_pixels, **kw):
    """Feed the streams' sequences through a chain of this layout until one runs out ->
    per stream the list of its rows."""
    chain = _Chain(counts, K, min_pixels, **kw)
    pos = [0] * len(seqs)
    got = [[] for _ in seqs]
    while all(pos[s] + c <= len(seqs[s]) for s, c in enumerate(counts)):
        maps, owner = [], []
        for s, c in enumerate(counts):
            maps += seqs[s][pos[s]:pos[s] + c]
            owner += [s] * c
            pos[s] += c
        for row, s in zip(chain.step(maps), owner):
            got[s].append(row)
    return got


def _same(got, want):
    assert len(got) == len(want) > 0
    for k, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g, w), (k, np.flatnonzero(g != w)[:8], g[:4], w[:4])


@functools.lru_cache(maxsize=None)
def _sequences():
    """Two streams' label maps: rectangles of several classes that drift, grow, split and meet,
    over sparse noise (so regions come and go around min_pixels and around K)."""
    out = []
    for seed, n in ((3, 8), (4, 4)):
        rng = np.random.default_rng(seed)
        rects = [(int(rng.integers(0, H - 12)), int(rng.integers(0, W - 16)), int(rng.integers(5, 14)),
                  int(rng.integers(6, 20)), int(rng.integers(1, 6)), int(rng.integers(-3, 4)),
                  int(rng.integers(-4, 5))) for _ in range(9)]
        seq = []
        for t in range(n):
            m = np.zeros((H, W), np.uint8)
            for y, x, h, w, c, vy, vx in rects:
                yy, xx = max(0, y + vy * t), max(0, x + vx * t)
                m[yy:yy + h + (t if c == 2 else 0), xx:xx + w] = c
            if t % 3 == 2:
                m[:, 30:32] = 0  # a gap splits what crosses it
            noise = rng.random(m.shape) < 0.03
            m[noise] = rng.integers(0, 6, int(noise.sum()))
            seq.append(m)
        out.append(seq)
    wants = [_oracle(seq, KS, 3) for seq in out]
    return out, wants


def test_the_sequences_exercise_the_definition():
    (s0, s1), (w0, w1) = _sequences()
    tabs = [RG.decode(w, tracks=True) for w in w0]
    assert all(int(w[0]) > KS for w in w0 + w1)               # more regions than K: some fall out
    assert max(int(t["age"].max()) for t in tabs) >= 4   # tracks that last
    assert sum(int((t["age"][1:] == 1).sum()) for t in tabs[1:]) > 0  # and new ones later on
    ids = [t["track_id"].tolist() for t in tabs]
    assert any(a != sorted(a) for a in ids)              # ids follow regions, not slots


def test_kernel_equals_the_oracle_in_every_batching():
    (s0, s1), (w0, w1) = _sequences()
    one = _run([s0], [1], KS, 3)[0]           # B = 1, 8 steps
    _same(one, w0)
    four = _run([s0], [4], KS, 3)[0]          # B = 4, one stream, 2 steps
    _same(four, w0)
    a, b = _run([s0, s1], [2, 2], KS, 3)      # B = 4, two streams
    _same(a, w0[:4])
    _same(b, w1)
    a, b = _run([s0, s1], [2, 1], KS, 3)      # B = 3: the streams advance at different rates
    _same(a, w0)
    _same(b, w1)
    _same(_run([s1], [3], KS, 3)[0], w1[:3])


def test_a_stream_without_a_row_keeps_its_state():
    (s0, s1), (w0, w1) = _sequences()
    hip = _hip()
    state = torch.zeros(hip.region_tracks_state_bytes(2, CH, CW), dtype=torch.uint8, device=DEV)
    both = _Chain([1, 1], KS, 3, state=state)
    only0 = _Chain([1, 0], KS, 3, state=state)   # split_batch(1, 2): stream 1 has no row
    got0, got1 = [], []
    r = both.step([s0[0], s1[0]])
    got0.append(r[0].copy()), got1.append(r[1].copy())
    got0.append(only0.step([s0[1]])[0].copy())
    got0.append(only0.step([s0[2]])[0].copy())
    r = both.step([s0[3], s1[1]])
    got0.append(r[0].copy()), got1.append(r[1].copy())
    _same(got0, w0[:4])
    _same(got1, w1[:2])


def _pair(m0, m1, K, mp, classes, geom=(H, W, CH, CW), third=None):
    """Two (three) frames of one stream, as B = 1 steps and as one batch: both equal the oracle."""
    seq = [m0, m1] + ([third] if third is not None else [])
    want = _oracle(seq, K, mp, classes, geom)
    _same(_run([seq], [1], K, mp, classes=classes, geom=geom)[0], want)
    _same(_run([seq], [len(seq)], K, mp, classes=classes, geom=geom)[0], want)
    return [RG.decode(w, tracks=True) for w in want]


def test_one_region_covers_the_crop_in_both_frames():
    m = np.full((H, W), 5, np.uint8)
    t0, t1 = _pair(m, m, 4, 1, [5])
    assert t0["pixels"].tolist() == [CH * CW] and (t1["track_id"][0], t1["age"][0]) == (1, 2)


def test_checkerboard():
    y, x = np.mgrid[:H, :W]
    cb = (1 + ((x + y) & 1)).astype(np.uint8)
    t0, t1, t2 = _pair(cb, cb, 4, 1, [1, 2], third=(3 - cb).astype(np.uint8))
    assert t1["track_id"].tolist() == [1, 2] and t1["age"].tolist() == [2, 2]
    assert t2["track_id"].tolist() == [3, 4] and t2["age"].tolist() == [1, 1]  # no shared pixel of one class


def test_all_singletons():
    y, x = np.mgrid[:H, :W]
    lab = (1 + (x & 1) + 2 * (y & 1)).astype(np.uint8)
    assert CH * CW <= _hip().REGION_CANDIDATES
    t0, t1 = _pair(lab, lab, 64, 1, [1, 2, 3, 4])
    assert len(t1) == 64 and t1["track_id"].tolist() == list(range(1, 65)) and (t1["age"] == 2).all()


def test_no_served_pixels_at_all():
    z = np.zeros((H, W), np.uint8)
    m = z.copy()
    m[3:9, 5:30] = 2
    seq = [z, m, z, m, m]
    want = _oracle(seq, 4, 1, [2])
    _same(_run([seq], [1], 4, 1, classes=[2])[0], want)
    _same(_run([seq], [5], 4, 1, classes=[2])[0], want)
    t = [RG.decode(w, tracks=True) for w in want]
    assert [x["track_id"].tolist() for x in t] == [[], [1], [], [2], [2]] and t[4]["age"].tolist() == [2]


def test_k_256_reaches_the_full_overlap_table():
    """A 64 x 64 crop of singletons, min_pixels 1: 4096 candidates, 256 stored; in the second
    frame some pairs have grown, so the slots shift and the ids follow the regions."""
    g = (66, 72, 64, 64)
    y, x = np.mgrid[:66, :72]
    a = (1 + (x & 1) + 2 * (y & 1)).astype(np.uint8)
    b = a.copy()
    b[0, 5] = a[0, 4]        # joins its two neighbours in the row: a three-pixel region, slot 0
    b[2, 2] = a[2, 1]        # and another, slot 1
    assert 64 * 64 == _hip().REGION_CANDIDATES
    t0, t1 = _pair(a, b, 256, 1, [1, 2, 3, 4], geom=g)
    assert len(t0) == len(t1) == 256 and t1["pixels"][:2].tolist() == [3, 3]
    # each overlaps two singletons of frame 0 by one pixel: the tie goes to the smaller slot
    assert t1["age"][:2].tolist() == [2, 2] and t1["track_id"][:2].tolist() == [5, 130]
    assert (t1["age"] == 2).sum() > 200
    assert (t1["age"] == 1).sum() > 0


@functools.lru_cache(maxsize=None)
def _shipped():
    rng = np.random.default_rng(4)
    coarse = rng.integers(0, 21, (33, 33)).astype(np.uint8)
    a = np.repeat(np.repeat(coarse, 16, 0), 16, 1)[:513, :513].copy()
    b = np.roll(a, (5, 9), (0, 1))
    b[200:260, :] = 7
    for m in (a, b):
        sp = rng.random(m.shape) < 0.02
        m[sp] = rng.integers(0, 21, int(sp.sum()))
    mp = RG.min_pixels_for(0.002, 513, 513)
    g = (513, 513, 385, 513)
    return a, b, mp, g, _oracle([a, b], 64, mp, RG.default_classes(21), g)


def test_shipped_geometry_pair():
    a, b, mp, g, want = _shipped()
    got = _run([[a, b]], [2], 64, mp, classes=RG.default_classes(21), geom=g)[0]
    _same(got, want)
    t = RG.decode(want[1], tracks=True)
    assert len(t) > 8 and (t["age"] == 2).sum() > 4 and (t["age"] == 1).sum() > 0


def test_wrapper_rejects_bad_arguments_without_launching():
    c = _Chain([2, 1], 8, 3)
    c.launch()
    torch.cuda.synchronize()
    c.out.fill_(SENT)
    before = c.state.clone()
    hip = _hip()
    ok = dict(rows=c.rows, out=c.out, ws=c.ws, tws=c.tws, state=c.state, tables=c.tables)
    kw = dict(counts=[2, 1], crop_h=CH, crop_w=CW, K=8, q=256)

    def go(exc, **ch):
        a, k = dict(ok), dict(kw)
        for name, v in ch.items():
            (a if name in a else k)[name] = v
        with pytest.raises(exc):
            hip.region_tracks(a["rows"], a["out"], a["ws"], a["tws"], a["state"], a["tables"], **k)

    go(TypeError, out=c.out.float())
    go(TypeError, tables=c.tables.long())
    go(ValueError, out=c.rows)                   # the narrow rows: wrong shape, and the same buffer
    go(ValueError, rows=c.out)
    go(ValueError, counts=[2, 2])                # B = 4: the buffers hold 3 rows
    go(ValueError, counts=[3])                   # one stream: state and tables are for two
    go(ValueError, counts=[])
    go(ValueError, counts=[4, -1])
    go(ValueError, K=0)
    go(ValueError, K=257)
    go(ValueError, K=7)
    go(ValueError, q=0)
    go(ValueError, q=1025)
    go(ValueError, crop_h=CH + 1)                # state is for another crop
    go(ValueError, ws=c.ws[:64])
    go(ValueError, tws=c.tws[:64])
    go(ValueError, state=c.state[:-4])
    go(ValueError, tables=c.tables[:-1])
    go(ValueError, conf=True)                    # 7-word rows expected
    go(ValueError, out=c.out.cpu())
    torch.cuda.synchronize()
    assert (c.out.cpu().numpy() == SENT).all() and torch.equal(c.state, before)


# ---- graph capture ------------------------------------------------------------------------------

def test_captured_state_persists_across_replays_and_resets():
    from semantic_segmentation_server_amd.postprocess.device import DevicePostprocess
    (s0, s1), (w0, w1) = _sequences()
    dev = torch.device(DEV)
    dp = DevicePostprocess(dev, H, W, np.zeros((256, 3), np.int32), K=8, bins=8, region_cap=KS,
                           region_classes=RG.class_mask(CLS), region_min_pixels=3, track_streams=2,
                           track_q=256)
    assert dp.out_words == 8 and dp.track_counts(2) == [1, 1]
    lab = torch.zeros((2, H, W), dtype=torch.uint8, device=dev)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        dp.run(lab, CW, CH, 4.0)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        dp.run(lab, CW, CH, 4.0)
    words = dp.last_regions
    assert tuple(words.shape) == (2, 4 + 8 * KS)

    def replay(k):
        lab.copy_(torch.from_numpy(np.stack([s0[k], s1[k]])))
        words.fill_(SENT)
        g.replay()
        torch.cuda.synchronize()
        return dp.fetch_regions(words)

    dp.reset_tracks()  # the warm-up run advanced the state
    for k in range(3):
        got = replay(k)
        assert np.array_equal(got[0], w0[k]) and np.array_equal(got[1], w1[k]), k
    assert RG.decode(w0[2], tracks=True)["age"].max() == 3
    dp.reset_tracks()
    got = replay(0)
    assert np.array_equal(got[0], w0[0]) and np.array_equal(got[1], w1[0])
    t = RG.decode(got[0], tracks=True)
    assert t["track_id"].tolist() == list(range(1, len(t) + 1)) and (t["age"] == 1).all()


# ---- engine and pipeline ------------------------------------------------------------------------

def _cfg(**kw):
    from semantic_segmentation_server_amd import config as C
    base = dict(input_size=129, batch=4, streams=2, backend="hip", graph=False, min_area_ratio=0.0005,
                serve_regions=True, track_regions=True)
    base.update(kw)
    return C.Config(**base)


@functools.lru_cache(maxsize=None)
def _frames():
    from semantic_segmentation_server_amd.runtime.sources import SyntheticSource
    src = SyntheticSource(160, 120, pool=3, seed=11)
    return [src.read_batch(1)[0][0].copy() for _ in range(3)]


def _batches(n):
    """n batches of 4 frames (rows 0, 1: stream 0; rows 2, 3: stream 1) from a pool of three
    images: a stream sees runs of one image (its regions continue) and changes of image."""
    P = _frames()
    out = []
    for k in range(n):
        a, b, c = P[(k // 2) % 3], P[(k + 1) % 3], P[(2 * k) % 3]
        out.append(torch.from_numpy(np.stack([a, a, b, c])))
    return out


def _engine_oracle(eng, batches, streams=(0, 0, 1, 1)):
    """Per stream, the rows of all its frames by the definition, from the engine's own label
    maps (and confidence planes) of every batch."""
    trk = {s: TK.StreamTracker(eng.track_q) for s in set(streams)}
    rw = eng.region_words
    rows = []
    for f in batches:
        labels, conf = eng._infer(f.to(DEV))
        torch.cuda.synchronize()
        labels = labels.cpu().numpy()
        conf = conf.cpu().numpy() if conf is not None else None
        rows.append(np.stack([
            RG.encode(labels[b], eng.crop_w, eng.crop_h, eng.region_mask, eng.region_min_pixels, eng.region_cap,
                      out=np.zeros(4 + rw * eng.region_cap, np.uint32), tracker=trk[streams[b]],
                      **({"conf": conf[b]} if conf is not None else {})) for b in range(len(streams))]))
    return rows


def _used(eng, row):
    return RG.used_words(row, eng.region_cap, conf=eng.serve_confidence, tracks=True)


def test_engine_graph_and_no_graph_give_the_oracles_words():
    from semantic_segmentation_server_amd.runtime.engine import Engine
    batches = _batches(4)
    got = {}
    for graph in (False, True):
        eng = Engine(_cfg(graph=graph), torch.device(DEV))
        assert eng.region_words == 8 and eng.track_streams == 2
        got[graph] = []
        for k, f in enumerate(batches):
            eng.step(f.numpy(), [4 * k + i for i in range(4)], [0.0] * 4, [6, 6, 2, 2])
            got[graph].append(eng.regions.copy())
        want = _engine_oracle(eng, batches)
        aged = 0
        for k in range(len(batches)):
            assert got[graph][k].shape == (4, 4 + 8 * 64)
            for b in range(4):
                u = _used(eng, want[k][b])
                assert np.array_equal(got[graph][k][b, :u], want[k][b, :u]), (graph, k, b)
                aged += int((RG.decode(want[k][b], tracks=True)["age"] > 1).sum())
        assert aged > 0
        with pytest.raises(ValueError, match="--track_regions"):
            eng.step(batches[0].numpy(), [0, 1, 2, 3], [0.0] * 4, [6, 2, 6, 2])
    for k in range(len(batches)):
        for b in range(4):
            u = _used(eng, got[True][k][b])
            assert np.array_equal(got[True][k][b, :u], got[False][k][b, :u])


def _drive(eng, batches, hub):
    from semantic_segmentation_server_amd.parallel import dist as D
    from semantic_segmentation_server_amd.parallel.dp import DataParallelPipeline
    pipe = DataParallelPipeline(D.init(), eng, 160, 120, 4, "local", hub, 2, lag=2)
    assert pipe.lag == 2 and pipe.nslots == 3 and eng.slot_parallel
    n = len(batches)
    out = []
    pipe.prefetch(batches[0].pin_memory())
    for k in range(n):
        out.append(pipe.step(frame_ids=[100 + 4 * k + i for i in range(4)], ts=[1.0 + k] * 4,
                             streams=[0, 0, 1, 1],
                             next_frames=batches[k + 1].pin_memory() if k + 1 < n else None))
    out.append(pipe.flush())
    torch.cuda.synchronize()
    return pipe, np.concatenate(out)


@pytest.mark.parametrize("conf", [False, True])
def test_pipeline_with_three_slots_equals_the_oracle_over_all_steps(conf):
    from semantic_segmentation_server_amd.runtime.engine import Engine
    from semantic_segmentation_server_amd.runtime.results import ResultHub
    n = 2 * 3 + 1
    batches = _batches(n)
    eng = Engine(_cfg(graph=True, serve_confidence=conf), torch.device(DEV))
    assert eng.region_words == 8 + conf
    hub = ResultHub(2, maxlen=100000)
    pipe, recs = _drive(eng, batches, hub)
    want = _engine_oracle(eng, batches)[-1]
    for s, row in ((0, 1), (1, 3)):
        r = hub.regions(s)
        assert r is not None and r.tracks and r.conf == conf and r.frame_id == 100 + 4 * (n - 1) + row
        u = _used(eng, want[row])
        assert len(r.words) == u and np.array_equal(r.words, want[row][:u]), s
        t = RG.decode(r.words, conf=conf, tracks=True)
        if s == 0:  # the stream's last two frames are one image: every region continued
            assert len(t) and (t["age"] >= 2).all()
    with pytest.raises(ValueError, match="--track_regions"):
        pipe.step(frame_ids=[0, 1, 2, 3], ts=[0.0] * 4, streams=[0, 1, 0, 1])


def test_flag_off_rows_are_the_parents_and_no_track_buffer_exists():
    from semantic_segmentation_server_amd.runtime.engine import Engine
    batches = _batches(2)
    off = Engine(_cfg(track_regions=False, graph=True), torch.device(DEV))
    on = Engine(_cfg(graph=True), torch.device(DEV))
    assert off.region_words == 6 and not off.track_regions
    for k, f in enumerate(batches):
        ids = [4 * k + i for i in range(4)]
        r_off = off.step(f.numpy(), ids, [0.0] * 4, [0, 0, 1, 1])
        r_on = on.step(f.numpy(), ids, [0.0] * 4, [0, 0, 1, 1])
        assert r_off.tobytes() == r_on.tobytes()
        labels = off._infer_eager(f.to(DEV)).cpu().numpy()
        for b in range(4):
            want = RG.encode(labels[b], off.crop_w, off.crop_h, off.region_mask, off.region_min_pixels, 64)
            u = RG.used_words(want)
            assert off.regions.shape == (4, 4 + 6 * 64)
            assert off.regions[b, :u].tobytes() == want[:u].tobytes()
            n = (u - 4) // 6
            assert np.array_equal(on.regions[b, 4:4 + 8 * n].reshape(n, 8)[:, :6], want[4:u].reshape(n, 6))
    post = off._hip_post
    assert post.track_streams == 0 and not post._track_bufs and not post._track_state
    assert post.out_words == 6 and on._hip_post._track_bufs and on._hip_post._track_state
