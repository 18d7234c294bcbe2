"""Device zone presence (csrc/hip/zone_presence.hip, and the slot-plane launch of
csrc/hip/class_regions.hip) against the numpy definition (postprocess/presence.py), and the engine
/ pipeline layers that carry its output.

Every comparison is exact on the uint32 words, and on the whole row: ``out`` is prefilled with a
sentinel (every word must be written) and the workspace is over-allocated by a sentinel tail that
must come back unchanged. Each case runs ``class_regions``, then ``region_tracks`` where it
applies, then ``zone_presence``, on static buffers. The base geometry derives from the chunk the
wrapper exports: a crop of 97 columns and a little over two chunks of flat pixels inside a larger
map of odd width whose pixels outside the crop hold a served class.
"""
import json

import numpy as np
import pytest
import torch

import presence_cases as PC
import region_cases as RC
from semantic_segmentation_server_amd.postprocess import presence as PR
from semantic_segmentation_server_amd.postprocess import regions as RG
from semantic_segmentation_server_amd.postprocess import tracks as TK
from semantic_segmentation_server_amd.postprocess import zones as ZN

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENT = PC.SENT
WS_SENT = 0xA5
WS_TAIL = 256
OUTSIDE = 1  # the class of every pixel outside the crop (served by every case that embeds)
Q = 512
MP = 5   # min_pixels of the base geometry: 169 * 97 // 5 regions fit the selection's candidates


def _hip():
    from semantic_segmentation_server_amd.ops import hip_ops
    return hip_ops


def _geom():
    """(H, W, crop_h, crop_w, chunk): 97 columns, a little over 2 chunks of flat pixels, inside
    a map 3 rows taller and 4 columns wider (odd width)."""
    chunk = _hip().zone_presence_chunk()
    cw = 97
    ch = -(-(2 * chunk + 9) // cw)
    assert cw * ch >= 2 * chunk + 9 and (cw + 4) % 2 == 1
    return ch + 3, cw + 4, ch, cw, chunk


def _canvas(inner, crop_h, crop_w, H=None, W=None):
    inner = np.asarray(inner, np.uint8)
    if inner.ndim == 2:
        inner = inner[None]
    H, W = H or crop_h + 3, W or crop_w + 4
    lab = np.full((inner.shape[0], H, W), OUTSIDE, np.uint8)
    lab[:, :crop_h, :crop_w] = inner
    return lab


class _Chain:
    """class_regions (+ region_tracks) + zone_presence on static buffers for one batch layout.
    ``counts``: the rows each stream owns (tracking), or the batch size (no tracking)."""

    def __init__(self, counts, K, min_pixels, classes, geom, R, plane=None, q=Q, track_q=256, state=None,
                 pstate=None):
        hip = _hip()
        self.tracks = not isinstance(counts, int)
        self.counts = list(counts) if self.tracks else None
        B = self.B = sum(counts) if self.tracks else counts
        self.K, self.mp, self.classes, self.R, self.q, self.track_q = K, min_pixels, classes, R, q, track_q
        self.H, self.W, self.ch, self.cw = geom
        self.lab = torch.zeros((B, self.H, self.W), dtype=torch.uint8, device=DEV)
        self.rows = torch.full((B, 4 + 6 * K), SENT, dtype=torch.int32, device=DEV)
        self.ws = torch.zeros(hip.class_regions_workspace_bytes(B, self.ch, self.cw), dtype=torch.uint8, device=DEV)
        self.plane = torch.zeros((self.ch, self.cw), dtype=torch.int32, device=DEV) if R > 1 else None
        if plane is not None:
            self.set_plane(plane)
        self.out = torch.full((B, PR.frame_words(K, R, self.tracks)), SENT, dtype=torch.int32, device=DEV)
        self.nb = hip.zone_presence_workspace_bytes(B, self.ch, self.cw, self.tracks)
        self.pws = torch.full((self.nb + WS_TAIL,), WS_SENT, dtype=torch.uint8, device=DEV)
        if self.tracks:
            S = len(counts)
            self.wide = torch.full((B, 4 + 8 * K), SENT, dtype=torch.int32, device=DEV)
            self.tws = torch.zeros(hip.region_tracks_workspace_bytes(B, self.ch, self.cw, K), dtype=torch.uint8,
                                   device=DEV)
            self.state = state if state is not None else torch.zeros(
                hip.region_tracks_state_bytes(S, self.ch, self.cw), dtype=torch.uint8, device=DEV)
            self.pstate = pstate if pstate is not None else torch.zeros(
                hip.zone_presence_state_bytes(S, K, R), dtype=torch.uint8, device=DEV)
            self.tables = hip.region_track_tables(counts, DEV)

    def set_plane(self, plane):
        self.plane.copy_(torch.from_numpy(np.ascontiguousarray(plane, np.uint32).view(np.int32)))

    def launch(self):
        hip = _hip()
        hip.class_regions(self.lab, self.rows, self.ws, B=self.B, H=self.H, W=self.W, crop_h=self.ch,
                          crop_w=self.cw, classes=self.classes, min_pixels=self.mp, K=self.K)
        kw = {}
        if self.tracks:
            hip.region_tracks(self.rows, self.wide, self.ws, self.tws, self.state, self.tables,
                              counts=self.counts, crop_h=self.ch, crop_w=self.cw, K=self.K, q=self.track_q)
            kw = dict(tws=self.tws, state=self.pstate, tables=self.tables, counts=self.counts, q=self.q)
        hip.zone_presence(self.wide if self.tracks else self.rows, self.out, self.pws, self.ws, B=self.B,
                          crop_h=self.ch, crop_w=self.cw, K=self.K, R=self.R, plane=self.plane, **kw)

    def load(self, maps):
        self.lab.copy_(torch.from_numpy(np.ascontiguousarray(np.stack(maps), np.uint8)))

    def step(self, maps):
        """One batch (its B maps in row order) -> (region rows as served, presence rows), uint32."""
        self.load(maps)
        self.out.fill_(SENT)
        self.launch()
        torch.cuda.synchronize()
        assert (self.pws[self.nb:].cpu().numpy() == WS_SENT).all()
        rows = self.wide if self.tracks else self.rows
        return rows.cpu().numpy().view(np.uint32), self.out.cpu().numpy().view(np.uint32)


def _same_rows(got, want, what=""):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(got[:4], want[:4]), (what, got[:4], want[:4])
    assert np.array_equal(got, want), (what, np.flatnonzero(got != want)[:8])


def _check(labels, plane, ch, cw, R, K, mp, classes, q=Q, both=True):
    """Launch on ``labels`` [B, H, W], without tracking and (``both``) with it, every frame the
    first of a stream of its own: every word of every row equals the definition's. Returns the
    decoded frames of the run without tracking."""
    labels = np.ascontiguousarray(labels, np.uint8)
    B, H, W = labels.shape
    dec = None
    for tracks in ((False, True) if both else (False,)):
        chain = _Chain([1] * B if tracks else B, K, mp, classes, (H, W, ch, cw), R, plane, q)
        _, got = chain.step(list(labels))
        for b in range(B):
            (_, want), = PC.oracle([labels[b]], tracks, K, mp, classes, (ch, cw), plane, R, q)
            _same_rows(got[b], want, (tracks, b))
        if not tracks:
            dec = [PR.decode(g, R) for g in got]
    return dec


def _blocks(rng, crop_h, crop_w, C, speckle=0.02):
    """Piecewise-constant labels (random rectangles) plus speckle, all < C."""
    lab = np.full((crop_h, crop_w), rng.integers(C), np.uint8)
    for _ in range(6):
        y0, x0 = rng.integers(crop_h), rng.integers(crop_w)
        lab[y0:y0 + 1 + rng.integers(crop_h), x0:x0 + 1 + rng.integers(crop_w)] = rng.integers(C)
    m = rng.random((crop_h, crop_w)) < speckle
    lab[m] = rng.integers(C, size=int(m.sum()))
    return lab


# ---- kernel ----------------------------------------------------------------------------------------

def test_one_region_over_the_whole_crop_in_all_32_zones():
    """Maximum contention: every run adds to 33 counters of one region, and every counter equals N."""
    H, W, ch, cw, _ = _geom()
    plane = np.full((ch, cw), 0xFFFFFFFF, np.uint32)
    (p,) = _check(_canvas(np.full((ch, cw), 7, np.uint8), ch, cw, H, W), plane, ch, cw, 33, 4, MP, [1, 7])
    assert p.n == 1 and (p.P == ch * cw).all() and p.label[0] == 7 and p.root[0] == 0


def test_256_stored_regions_in_32_zones_fill_the_table():
    """3 x 2 blocks at pitch (4, 3): 1344 regions of 6 px, ordered by root; K = 256 of them stored."""
    H, W, ch, cw, _ = _geom()
    assert (ch, cw) == (169, 97)
    lab = np.zeros((ch, cw), np.uint8)
    n = 0
    for y0 in range(0, ch - 2, 4):
        for x0 in range(0, cw - 1, 3):
            lab[y0:y0 + 3, x0:x0 + 2] = 2 + (n % 3)
            n += 1
    assert n == 1344
    RG.check_geometry(cw, ch, 5, 256)
    rng = np.random.default_rng(1)
    plane = rng.integers(0, 1 << 32, (ch, cw), dtype=np.uint64).astype(np.uint32)
    plane[:8] = 0xFFFFFFFF
    (p,) = _check(_canvas(lab, ch, cw, H, W), plane, ch, cw, 33, 256, 5, [2, 3, 4])
    assert p.n == 256 and (p.P[:, 0] == 6).all() and (np.diff(p.root.astype(np.int64)) > 0).all()
    assert (p.P[:32] == 6).all() and p.P[:, 1:].max() == 6 and p.P[32:, 1:].min() == 0


def test_checkerboard_of_two_classes_against_striped_zones_has_no_runs():
    H, W, ch, cw, _ = _geom()
    y, x = np.mgrid[:ch, :cw]
    lab = (2 + ((x + y) & 1)).astype(np.uint8)
    plane = ((x % 3 == 0) | ((x % 3 == 1) << 1) | ((y % 2) << 2) | (((x + 2 * y) % 5 == 0) << 3)).astype(np.uint32)
    (p,) = _check(_canvas(lab, ch, cw, H, W), plane, ch, cw, 5, 8, MP, [2, 3])
    assert p.n == 2 and p.P[:, 0].sum() == ch * cw   # 8-connected: each colour is one region


def test_single_pixel_zones_at_every_boundary():
    H, W, ch, cw, chunk = _geom()
    n = ch * cw
    flat = [0, n - 1, chunk - 1, chunk, 2 * chunk - 1, 2 * chunk, 63, 64, 64 * 32 - 1, 64 * 32,
            cw - 1, cw, 5 * cw - 1, 5 * cw, (ch - 1) * cw - 1, (ch - 1) * cw, chunk + 63, chunk + 64]
    assert len(set(flat)) == len(flat) <= 32 and max(flat) < n
    plane = np.zeros(n, np.uint32)
    for k, i in enumerate(flat):
        plane[i] |= np.uint32(1) << np.uint32(k)
    plane = plane.reshape(ch, cw)
    rng = np.random.default_rng(2)
    lab = _blocks(rng, ch, cw, 6, speckle=0.0)
    (p,) = _check(_canvas(lab, ch, cw, H, W), plane, ch, cw, 1 + len(flat), 64, MP, list(range(6)))
    slots = TK.slot_plane(lab, cw, ch, list(range(6)), MP, 64)
    stored = [int(slots[i] != TK.NONE) for i in flat]   # a zone's pixel counts once, if a stored region holds it
    assert p.P[:, 1:].sum(0).tolist() == stored and sum(stored) >= len(flat) - 2


def test_pixels_that_count_nowhere():
    """Regions past K, regions below min_pixels and an unserved class: none of their pixels is
    counted, in any row."""
    H, W, ch, cw, _ = _geom()
    rng = np.random.default_rng(3)
    lab = _blocks(rng, ch, cw, 6, speckle=0.03)
    plane = rng.integers(0, 16, (ch, cw)).astype(np.uint32)
    K, mp, classes = 3, MP, [1, 2, 3, 4]
    tab = RG.region_table(lab, cw, ch, classes, mp)
    small = RG.region_table(lab, cw, ch, classes, 1)
    assert len(tab) > K and len(small) > len(tab) and np.isin(lab, [0, 5]).any()
    (p,) = _check(_canvas(lab, ch, cw, H, W), plane, ch, cw, 5, K, mp, classes)
    assert p.n == K and p.P[:, 0].tolist() == tab["pixels"][:K].tolist() and p.P[:, 0].sum() < np.isin(lab, classes).sum()


def test_a_frame_with_no_region_is_header_and_zeros():
    H, W, ch, cw, _ = _geom()
    lab = np.full((ch, cw), 9, np.uint8)
    lab[::2, ::2] = 2          # served, but every component is one pixel: below min_pixels
    y, x = np.mgrid[:ch, :cw]
    two = np.stack([lab, (2 + ((x + y) & 1)).astype(np.uint8)])   # and a frame with regions beside it
    dec = _check(_canvas(two, ch, cw, H, W), np.full((ch, cw), 5, np.uint32), ch, cw, 4, 8, MP, [2, 3])
    assert dec[0].n == 0 and dec[1].n == 2


@pytest.mark.parametrize("crop", [(1, 1), (1, 200), (200, 1), (9, 63), (9, 64), (9, 65), (5, 255), (5, 256),
                                  (5, 257)])
def test_thin_and_wave_sized_crops(crop):
    ch, cw = crop
    rng = np.random.default_rng(100 * ch + cw)
    lab = _blocks(rng, ch, cw, 5, speckle=0.1)
    plane = rng.integers(0, 4, (ch, cw)).astype(np.uint32)
    dec = _check(_canvas(np.stack([lab, lab[::-1, ::-1]]), ch, cw), plane, ch, cw, 3, 16, 1, [1, 2, 3, 4])
    assert np.isin(lab, [1, 2, 3, 4]).sum() >= dec[0].P[:, 0].sum()


@pytest.mark.parametrize("column", [False, True])
def test_the_two_16_bit_limit_crops(column):
    """1 x 65535 and 65535 x 1 (tests/region_cases.py): frame 0 is one region over the crop, so its
    counts are the zones' sizes in closed form; frame 1 holds more regions than K."""
    b = RC.build_limit(column)
    n = RC.LIMIT
    i = np.arange(n, dtype=np.int64)
    plane = ((i < 1000).astype(np.uint32) | ((i >= n - 5).astype(np.uint32) << 31) |
             (((i // 64) % 2).astype(np.uint32) << 7) | np.uint32(2)).reshape(b.crop_h, b.crop_w)
    dec = _check(b.labels, plane, b.crop_h, b.crop_w, 33, b.K, b.min_pixels, list(b.classes))
    want = np.zeros(33, np.int64)
    want[[0, 1, 2, 8, 32]] = (n, 1000, n, int(((i // 64) % 2).sum()), 5)
    assert dec[0].n == 1 and dec[0].P[0].tolist() == want.tolist() and dec[1].n == b.K


def test_the_shipped_513_x_384_crop():
    rng = np.random.default_rng(4)
    ch, cw = 384, 513
    from semantic_segmentation_server_amd.postprocess import synthetic
    lab = np.stack([synthetic.random_label_map(rng, 513, 513) for _ in range(2)]).astype(np.uint8)
    plane = PC.zone_plane(cw, ch)
    mp = RG.min_pixels_for(0.002, 513, 513)
    dec = _check(lab, plane, ch, cw, 4, 64, mp, list(range(1, 21)))
    for p in dec:
        assert p.n > 0 and np.array_equal(p.P[:, 1] + p.P[:, 2], p.P[:, 0])


def test_seeded_random_cases():
    """200 tiny cases: random crop, Z, K, batch and classes, with and without tracks."""
    rng = np.random.default_rng(2024)
    for case in range(200):
        ch, cw = int(rng.integers(1, 40)), int(rng.integers(1, 150))
        Z, K, B = int(rng.integers(0, 6)), int(rng.integers(1, 12)), int(rng.integers(1, 4))
        zl = []
        for k in range(Z):
            pts = rng.uniform(-0.2, 1.2, (3, 2))
            if k % 2:
                (x0, y0), (x1, y1) = pts[0], pts[1]
                pts = np.array([[x0, y0], [x1, y0], [x1, y1], [x0, y1]])
            zl.append(ZN.Zone(f"z{k}", tuple(map(tuple, pts.tolist()))))
        plane = ZN.rasterize(zl, cw, ch, warn=False) if Z else None
        classes = sorted(set(int(c) for c in rng.integers(0, 7, int(rng.integers(1, 5))))) + [OUTSIDE]
        lab = np.stack([_blocks(rng, ch, cw, 8, speckle=0.05) for _ in range(B)])
        mp = max(int(rng.integers(1, 5)), ch * cw // RG.REGION_CANDIDATES + 1)
        _check(_canvas(lab, ch, cw), plane, ch, cw, 1 + Z, K, mp, classes,
               q=int(rng.integers(1, 1025)))


def test_three_frame_kinds_in_every_batch_position_share_one_plane():
    H, W, ch, cw, _ = _geom()
    rng = np.random.default_rng(8)
    y, x = np.mgrid[:ch, :cw]
    kinds = [np.full((ch, cw), 3, np.uint8), (1 + ((x + y) & 1)).astype(np.uint8), _blocks(rng, ch, cw, 9)]
    plane = ZN.rasterize([ZN.Zone("r", ((0.2, 0.3), (0.9, 0.3), (0.9, 0.8), (0.2, 0.8))),
                          ZN.Zone("t", ((0.0, 0.0), (1.0, 0.5), (0.0, 1.0)))], cw, ch)
    for rot in range(3):
        order = [kinds[(rot + k) % 3] for k in range(3)]
        _check(_canvas(np.stack(order), ch, cw, H, W), plane, ch, cw, 3, 8, MP, [1, 2, 3, 4, 5])


# ---- dwell -----------------------------------------------------------------------------------------

SGEOM = (PC.SH, PC.SW, PC.SCH, PC.SCW)


def _seq_chain(counts, **kw):
    return _Chain(counts, PC.SK, PC.SMP, PC.SCLS, SGEOM, 4, PC.zone_plane(PC.SCW, PC.SCH), PC.PRESENCE_Q,
                  PC.TRACK_Q, **kw)


def _run(seqs, counts):
    """Feed the streams' sequences through a chain of this layout until one runs out -> per
    stream the list of its (region row, presence row)."""
    chain = _seq_chain(counts)
    pos = [0] * len(seqs)
    got = [[] for _ in seqs]
    while all(pos[s] + c <= len(seqs[s]) for s, c in enumerate(counts)):
        maps, owner = [], []
        for s, c in enumerate(counts):
            maps += seqs[s][pos[s]:pos[s] + c]
            owner += [s] * c
            pos[s] += c
        rows, pres = chain.step(maps)
        for r, p, s in zip(rows, pres, owner):
            got[s].append((r.copy(), p.copy()))
    return got


def _same(got, want):
    assert len(got) == len(want) > 0
    for k, ((gr, gp), (wr, wp)) in enumerate(zip(got, want)):
        _same_rows(gr, wr, ("regions", k))
        _same_rows(gp, wp, ("presence", k))
        tab, p = RG.decode(gr, tracks=True), PR.decode(gp, 4, tracks=True)
        assert np.array_equal(p.P[:, 0], tab["pixels"]) and np.array_equal(p.D[:, 0], tab["age"])
        assert np.array_equal(p.P[:, 1] + p.P[:, 2], p.P[:, 0])


def test_the_sequences_exercise_the_definition():
    """On the oracle alone: what the dwell comparisons below are meant to see is in the sequences."""
    o0, _ = PC.sequence_oracles()
    block = []
    for reg, w in o0:
        p = PR.decode(w, 4, tracks=True)
        a = int(np.flatnonzero(p.track_id == 1)[0])
        block.append((p.P[a].tolist(), p.D[a].tolist()))
    left = [d[1] for _, d in block]
    assert max(left) >= 3                                          # a dwell >= 3
    assert left[5] == 0 and block[5][1][0] == 6                    # a leave while the age goes on
    assert left[6] == 1 and block[6][1][0] == 7                    # a re-entry
    assert 1024 * block[4][0][1] == PC.PRESENCE_Q * block[4][0][0] and left[4] == 5     # exactly at the threshold
    assert block[5][0][:3] == [100, 49, 51]                        # one pixel below it
    last = PR.decode(o0[7][1], 4, tracks=True)
    assert block[7][0][0] == 60 and block[7][1][2] == 4 and 30 in last.P[:, 0].tolist()  # a split: the larger inherits


def test_kernel_equals_the_oracle_in_every_batching():
    s0, s1 = (list(s) for s in PC.sequences())
    w0, w1 = PC.sequence_oracles()
    _same(_run([s0], [1])[0], w0)             # B = 1, 8 steps
    _same(_run([s0], [4])[0], w0)             # B = 4, one stream, 2 steps
    a, b = _run([s0, s1], [2, 2])             # B = 4, two streams
    _same(a, w0[:4])
    _same(b, w1)
    a, b = _run([s0, s1], [2, 1])             # B = 3: the streams advance at different rates
    _same(a, w0)
    _same(b, w1)
    _same(_run([s1], [3])[0], w1[:3])


def test_a_stream_without_a_row_keeps_its_dwell_and_reset_clears_it():
    s0, s1 = PC.sequences()
    w0, w1 = PC.sequence_oracles()
    hip = _hip()
    state = torch.zeros(hip.region_tracks_state_bytes(2, PC.SCH, PC.SCW), dtype=torch.uint8, device=DEV)
    pstate = torch.zeros(hip.zone_presence_state_bytes(2, PC.SK, 4), dtype=torch.uint8, device=DEV)
    both = _seq_chain([1, 1], state=state, pstate=pstate)
    only0 = _seq_chain([1, 0], state=state, pstate=pstate)   # split_batch(1, 2): stream 1 has no row
    got0, got1 = [], []

    def take(chain, maps, *into):
        rows, pres = chain.step(maps)
        for k, g in enumerate(into):
            g.append((rows[k].copy(), pres[k].copy()))

    take(both, [s0[0], s1[0]], got0, got1)
    take(only0, [s0[1]], got0)
    take(only0, [s0[2]], got0)
    take(both, [s0[3], s1[1]], got0, got1)
    _same(got0, w0[:4])
    _same(got1, w1[:2])
    assert pstate.any()
    state.zero_()
    pstate.zero_()                           # a reset: both streams start again
    got0, got1 = [], []
    take(both, [s0[0], s1[0]], got0, got1)
    take(both, [s0[1], s1[1]], got0, got1)
    _same(got0, w0[:2])
    _same(got1, w1[:2])


def test_reused_buffers_and_graph_replay_on_new_contents():
    """Without tracking: two runs on the same buffers with different labels and planes, then a
    captured graph replayed on new contents. With tracking: the captured chain replayed over the
    sequences keeps its dwell state from replay to replay."""
    H, W, ch, cw, _ = _geom()
    rng = np.random.default_rng(9)
    K, R, mp, classes = 12, 4, MP, [1, 2, 3, 4]
    chain = _Chain(2, K, mp, classes, (H, W, ch, cw), R, np.zeros((ch, cw), np.uint32))

    def contents():
        lab = _canvas(np.stack([_blocks(rng, ch, cw, 6) for _ in range(2)]), ch, cw, H, W)
        plane = (rng.integers(0, 8, (ch, cw)) * (rng.random((ch, cw)) < 0.5)).astype(np.uint32)
        return lab, plane

    def verify(lab, plane):
        got = chain.out.cpu().numpy().view(np.uint32)
        for b in range(2):
            _same_rows(got[b], PR.encode(lab[b], plane, cw, ch, classes, mp, K, R, Q), b)

    for _ in range(2):
        lab, plane = contents()
        chain.set_plane(plane)
        chain.step(list(lab))
        verify(lab, plane)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g):
            chain.launch()
    torch.cuda.current_stream().wait_stream(s)
    for _ in range(3):
        lab, plane = contents()
        chain.set_plane(plane)
        chain.load(list(lab))
        chain.out.fill_(SENT)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        verify(lab, plane)
    assert (chain.pws[chain.nb:].cpu().numpy() == WS_SENT).all()
    # tracking: state persists across the replays of one captured chain
    s0, _ = PC.sequences()
    w0, _ = PC.sequence_oracles()
    tchain = _seq_chain([2])
    tchain.load(s0[0:2])
    tchain.launch()                       # warm-up outside capture; it advances the state:
    torch.cuda.synchronize()
    tchain.state.zero_()
    tchain.pstate.zero_()                 # reset before the captured runs
    s.wait_stream(torch.cuda.current_stream())
    g2 = torch.cuda.CUDAGraph()
    tchain.load(s0[0:2])
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g2):
            tchain.launch()
    torch.cuda.current_stream().wait_stream(s)
    got = []
    for k in range(4):
        tchain.load(s0[2 * k:2 * k + 2])
        tchain.out.fill_(SENT)
        torch.cuda.synchronize()
        g2.replay()
        torch.cuda.synchronize()
        rows, pres = tchain.wide.cpu().numpy().view(np.uint32), tchain.out.cpu().numpy().view(np.uint32)
        got += [(rows[0].copy(), pres[0].copy()), (rows[1].copy(), pres[1].copy())]
    _same(got, w0)


def test_wrapper_rejects_bad_arguments_without_launching():
    hip = _hip()
    ch, cw, K, R = 8, 11, 4, 3
    c = _Chain(1, K, 1, [1], (9, 12, ch, cw), R, np.zeros((ch, cw), np.uint32))
    t = _Chain([1], K, 1, [1], (9, 12, ch, cw), R, np.zeros((ch, cw), np.uint32))

    def go(exc, chain=c, **kw):
        a = dict(rows=chain.wide if chain.tracks else chain.rows, out=chain.out, ws=chain.pws, cr_ws=chain.ws,
                 B=1, crop_h=ch, crop_w=cw, K=K, R=R, plane=chain.plane, conf=False)
        if chain.tracks:
            a.update(tws=chain.tws, state=chain.pstate, tables=chain.tables, counts=[1], q=Q)
        a.update(kw)
        pos = [a.pop(k) for k in ("rows", "out", "ws", "cr_ws")]
        with pytest.raises(exc):
            hip.zone_presence(*pos, **a)

    go(ValueError, rows=c.rows.cpu())
    go(TypeError, rows=c.rows.float())
    go(ValueError, rows=c.wide if c.tracks else torch.zeros((1, 4 + 8 * K), dtype=torch.int32, device=DEV))
    go(ValueError, conf=True)                   # 7-word records: the rows are 6 words wide
    go(TypeError, out=c.out.float())
    go(ValueError, out=t.out)                   # the tracking shape without tracking
    go(ValueError, out=c.rows, rows=c.rows, K=K, R=4)   # rows and out are one buffer (U = 6)
    wide = torch.full((1, 2 * c.out.shape[1]), SENT, dtype=torch.int32, device=DEV)
    go(ValueError, out=wide[:, ::2])
    go(ValueError, crop_h=0)
    go(ValueError, crop_h=4096, crop_w=4096)    # N = 2^24
    go(ValueError, K=0)
    go(ValueError, K=257)
    go(ValueError, R=0)
    go(ValueError, R=34)
    go(ValueError, plane=None)                  # R > 1 needs a plane
    go(ValueError, R=1, out=torch.full((1, 4 + 3 * K), SENT, dtype=torch.int32, device=DEV))  # R == 1 takes none
    go(TypeError, plane=c.plane.float())
    go(ValueError, plane=c.plane[:7])
    go(ValueError, plane=c.plane.cpu())
    go(TypeError, ws=c.pws.to(torch.int32))
    go(ValueError, ws=c.pws[:c.nb - 1])         # too small
    go(ValueError, ws=c.pws.cpu())
    go(ValueError, cr_ws=c.ws[:-1])
    go(ValueError, B=2)
    go(ValueError, B=0)
    go(ValueError, tws=t.tws)                   # the tracking arguments go together
    go(ValueError, q=Q)
    go(ValueError, chain=t, q=0)
    go(ValueError, chain=t, q=1025)
    go(ValueError, chain=t, counts=[2])
    go(ValueError, chain=t, counts=[1, 0])      # two streams: state and tables are for one
    go(ValueError, chain=t, counts=[])
    go(ValueError, chain=t, state=t.pstate[:-4])
    go(ValueError, chain=t, tables=t.tables[:-1])
    go(TypeError, chain=t, tables=t.tables.float())
    go(ValueError, chain=t, tws=t.tws[:-1])
    go(ValueError, chain=t, out=c.out)          # the shape without tracking
    go(ValueError, chain=t, rows=c.rows)        # the rows without tracks
    torch.cuda.synchronize()
    for ch_ in (c, t):
        assert (ch_.out.cpu().numpy() == SENT).all() and (ch_.pws.cpu().numpy() == WS_SENT).all()
    assert (wide.cpu().numpy() == SENT).all() and not t.pstate.any()


# ---- engine and pipeline ---------------------------------------------------------------------------

@pytest.fixture(scope="module")
def zone_file(tmp_path_factory):
    p = tmp_path_factory.mktemp("presence") / "zones.json"
    p.write_text(json.dumps(PC.ZONES))
    return str(p)


def _cfg(**kw):
    from semantic_segmentation_server_amd import config as C
    base = dict(input_size=129, batch=2, backend="hip", graph=False, min_area_ratio=0.0005)
    base.update(kw)
    return C.Config(**base)


def _on(zone_file, **kw):
    return _cfg(serve_regions=True, max_regions=8, serve_zones=True, zones=zone_file, serve_presence=True, **kw)


class _Oracle:
    """The presence rows of the engine's own label maps, frame after frame (one tracker and one
    dwell state per stream, as the engine's device state)."""

    def __init__(self, eng):
        self.eng = eng
        self.trk = {s: TK.StreamTracker(eng.track_q) for s in (0, 1)} if eng.track_regions else None
        self.dw = {s: PR.StreamDwell() for s in (0, 1)}

    def rows(self, frames, streams=(0, 1)):
        eng = self.eng
        labels, conf = eng._infer(frames.to(DEV))
        torch.cuda.synchronize()
        labels = labels.cpu().numpy()
        conf = conf.cpu().numpy() if conf is not None else None
        out = []
        for b, s in enumerate(streams):
            tab = None
            if self.trk is not None:
                reg = RG.encode(labels[b], eng.crop_w, eng.crop_h, eng.region_mask, eng.region_min_pixels,
                                eng.region_cap, conf=None if conf is None else conf[b], tracker=self.trk[s])
                tab = RG.decode(reg, conf=conf is not None, tracks=True)
            out.append(PR.encode(labels[b], eng.zone_plane, eng.crop_w, eng.crop_h, eng.region_mask,
                                 eng.region_min_pixels, eng.region_cap, eng.presence_rows, eng.presence_q,
                                 tab=tab, dwell=self.dw[s] if self.trk is not None else None))
        return np.stack(out)


@pytest.mark.parametrize("tracks", [False, True])
@pytest.mark.parametrize("graph", [False, True])
def test_engine_step_presence_is_that_of_its_labels(graph, tracks, zone_file):
    from semantic_segmentation_server_amd.runtime.engine import Engine
    from semantic_segmentation_server_amd.runtime.sources import SyntheticSource
    eng = Engine(_on(zone_file, graph=graph, track_regions=tracks, streams=2), torch.device(DEV))
    assert eng.presence_rows == 4 and eng.presence_unit == PR.unit(4, tracks) and eng.presence_q == 512
    src = SyntheticSource(200, 150, pool=6, seed=7)
    first, _, _ = src.read_batch(2)
    eng.step(first, [0, 1], [1.0, 2.0], [0, 1])   # builds (and with graph captures) the step:
    eng.reset_tracks()                            # warm-up and capture advance the state
    orc = _Oracle(eng)
    seen = 0
    for k in range(3):
        f, _, _ = src.read_batch(2)
        eng.step(f, [2 * k, 2 * k + 1], [1.0, 2.0], [0, 1])
        got = eng.presence.copy()
        assert got.shape == (2, 4 + eng.presence_unit * 8) and got.dtype == np.uint32
        want = orc.rows(torch.from_numpy(f))
        for b in range(2):
            _same_rows(got[b], want[b], (k, b))
            p = PR.decode(got[b], 4, tracks)
            rt = RG.decode(eng.regions[b], tracks=tracks)
            assert np.array_equal(p.P[:, 0], rt["pixels"]) and np.array_equal(p.P[:, 1] + p.P[:, 2], p.P[:, 0])
            seen += p.n
    assert seen > 0


def _drive(eng, batches, hub):
    from semantic_segmentation_server_amd.parallel import dist as D
    from semantic_segmentation_server_amd.parallel.dp import DataParallelPipeline
    pipe = DataParallelPipeline(D.init(), eng, 160, 120, 2, "local", hub, 2, lag=2)
    assert pipe.lag == 2 and pipe.nslots == 3 and eng.slot_parallel
    n = len(batches)
    out = []
    pipe.prefetch(batches[0].pin_memory())
    for k in range(n):
        out.append(pipe.step(frame_ids=[100 + 2 * k, 101 + 2 * k], ts=[1.0 + k, 1.5 + k], streams=[0, 1],
                             next_frames=batches[k + 1].pin_memory() if k + 1 < n else None))
    out.append(pipe.flush())
    torch.cuda.synchronize()
    return pipe, np.concatenate(out)


def _batches(n):
    from semantic_segmentation_server_amd.runtime.sources import SyntheticSource
    src = SyntheticSource(160, 120, pool=2 * n, seed=11)
    batches = [torch.from_numpy(src.read_batch(2)[0].copy()) for _ in range(n)]
    assert len({b.numpy().tobytes() for b in batches}) == n
    return batches


def test_pipeline_pushes_the_latest_presence_and_flag_off_is_the_parent(zone_file):
    from semantic_segmentation_server_amd.runtime.engine import Engine
    from semantic_segmentation_server_amd.runtime.results import ResultHub
    n = 2 * 3 + 1  # 2 * nslots + 1
    batches = _batches(n)
    eng = Engine(_on(zone_file, graph=True, track_regions=True, streams=2), torch.device(DEV))
    hub = ResultHub(2, maxlen=100000)
    pipe, recs = _drive(eng, batches, hub)
    orc = _Oracle(eng)
    for f in batches:
        want = orc.rows(f)
    for s in range(2):
        z = hub.presence(s)
        assert z is not None and z.tracks and z.frame_id == 100 + 2 * (n - 1) + s and z.ts == n + 0.5 * s
        u = PR.used_words(want[s], 4, True)
        assert len(z.words) == u and np.array_equal(z.words, want[s][:u])   # only the used entries travel
        assert not want[s][u:].any()
    reg_on = [hub.regions(s).words.copy() for s in range(2)]
    zon_on = [hub.zones(s).words.copy() for s in range(2)]
    # flag off: no launch, no buffer, and records, regions and zones are bit-equal to the run with presence
    off = Engine(_cfg(graph=True, serve_regions=True, max_regions=8, serve_zones=True, zones=zone_file,
                      track_regions=True, streams=2), torch.device(DEV))
    hub_off = ResultHub(2, maxlen=100000)
    pipe_off, recs_off = _drive(off, batches, hub_off)
    assert off.presence_rows == 0 and off.presence_packed is None and off.presence is None
    assert pipe_off.local_presence is None and hub_off.presence(0) is None
    post = off._hip_post
    assert post.presence_rows == 0 and not post._presence_bufs and not post._presence_state and post.last_presence is None
    assert len(recs) > 0 and recs.tobytes() == recs_off.tobytes()
    for s in range(2):
        assert np.array_equal(hub_off.regions(s).words, reg_on[s]) and np.array_equal(hub_off.zones(s).words, zon_on[s])


@pytest.mark.parametrize("graph", [False, True])
def test_masks_regions_confidence_tracks_zones_and_presence_together(graph, zone_file):
    from semantic_segmentation_server_amd.postprocess import mask_rle as MR
    from semantic_segmentation_server_amd.runtime.engine import Engine
    eng = Engine(_on(zone_file, graph=graph, serve_masks=True, mask_max_runs=4096, serve_confidence=True,
                     track_regions=True, streams=2), torch.device(DEV))
    batches = _batches(4)
    eng.step(batches[0].numpy(), [0, 1], [0.0, 0.0], [0, 1])
    eng.reset_tracks()
    trk = {s: TK.StreamTracker(eng.track_q) for s in (0, 1)}
    dw = {s: PR.StreamDwell() for s in (0, 1)}
    for k, f in enumerate(batches[1:]):
        eng.step(f.numpy(), [2 * k, 2 * k + 1], [0.0, 0.0], [0, 1])
        presence, zones, regions, masks = eng.presence.copy(), eng.zones.copy(), eng.regions.copy(), eng.masks.copy()
        labels, conf = eng._infer(f.to(DEV))
        torch.cuda.synchronize()
        labels, conf = labels.cpu().numpy(), conf.cpu().numpy()
        for b in range(2):
            wz = ZN.encode(labels[b], eng.zone_plane, eng.crop_w, eng.crop_h, eng.zone_classes, rows=eng.zone_rows,
                           conf=conf[b])
            assert np.array_equal(zones[b], wz), (k, b)
            wr = RG.encode(labels[b], eng.crop_w, eng.crop_h, eng.region_mask, eng.region_min_pixels,
                           eng.region_cap, out=np.zeros(4 + eng.region_words * eng.region_cap, np.uint32),
                           tracker=trk[b], conf=conf[b])
            u = RG.used_words(wr, eng.region_cap, conf=True, tracks=True)
            assert np.array_equal(regions[b, :u], wr[:u]), (k, b)
            wp = PR.encode(labels[b], eng.zone_plane, eng.crop_w, eng.crop_h, eng.region_mask,
                           eng.region_min_pixels, eng.region_cap, 4, eng.presence_q,
                           tab=RG.decode(wr, conf=True, tracks=True), dwell=dw[b])
            _same_rows(presence[b], wp, (k, b))
            wm = MR.encode(labels[b], eng.crop_w, eng.crop_h, eng.mask_cap)
            um = 4 + min(int(wm[0]), eng.mask_cap)
            assert np.array_equal(masks[b, :um], wm[:um]), (k, b)
