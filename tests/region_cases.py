"""Inputs of the class-region kernels (csrc/hip/class_regions.hip) at the neighbourhoods and
limit geometries where their hand-made case decisions can go wrong: the case table and the
helpers shared by tests/test_region_cases_cpu.py (a second oracle against the definition, and
every case's predicate) and tests/test_regions_paths_gpu.py (the device against the
definition, ``postprocess/regions.py`` ``encode``).

* ``flood_regions`` / ``flood_table`` / ``flood_encode``: a plain queue flood fill over the 8
  neighbours, pixel by pixel, and the region records built from it. ``regions.label_components``
  is min-label hooking, the idea of the kernels; this one shares nothing with either.
* The exhaustive windows: all 2^12 fillings of a 3 x 4 window with two served classes, at five
  places of a crop of (tile + 3) x (tile + 4).
* ``CASES``: crop shapes, the 16-bit coordinate limit, the selection sort, the statistics
  slots. Each case names the one device path it is listed for, and ``check`` asserts from the
  reference's root plane and the geometry alone the property that puts it there.

Every constant of the kernels comes from ``hip_ops.REGION_TILE_W/H``, ``REGION_CANDIDATES`` and
``REGION_MAX_K``. Nothing here touches a device.
"""
from collections import deque
from dataclasses import dataclass
from math import isqrt
from typing import Callable, Tuple

import numpy as np

from semantic_segmentation_server_amd.ops import hip_ops
from semantic_segmentation_server_amd.postprocess import regions as RG

TW, TH = hip_ops.REGION_TILE_W, hip_ops.REGION_TILE_H
CAND = hip_ops.REGION_CANDIDATES
KMAX = hip_ops.REGION_MAX_K
BUCKETS = 16             # copies of a statistics slot (kBuckets of the kernel file; the CPU test reads it there)
SELECT_THREADS = 1024    # threads of k_cr_select (kSelThreads; the same)
SENT = 0x5A5A5A5A

N8 = ((-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1))
N4 = ((-1, 0), (0, -1), (0, 1), (1, 0))


# ------------------------------------------------------------------ the second oracle
def flood_regions(lab, mask, neighbours=N8):
    """[(label, [(y, x), ...]), ...]: the regions of the 2-D map ``lab`` for the served set
    ``mask``, by a queue flood fill from every unvisited served pixel in raster order (so a
    region's first pixel is its smallest flat index)."""
    L = np.asarray(lab).tolist()
    h, w = len(L), len(L[0])
    seen = [[False] * w for _ in range(h)]
    out = []
    for y in range(h):
        for x in range(w):
            c = L[y][x]
            if seen[y][x] or not (mask >> c) & 1:
                continue
            seen[y][x] = True
            q = deque([(y, x)])
            px = []
            while q:
                cy, cx = q.popleft()
                px.append((cy, cx))
                for dy, dx in neighbours:
                    ny, nx = cy + dy, cx + dx
                    if 0 <= ny < h and 0 <= nx < w and not seen[ny][nx] and L[ny][nx] == c:
                        seen[ny][nx] = True
                        q.append((ny, nx))
            out.append((c, px))
    return out


def flood_table(labels, crop_w, crop_h, classes, min_pixels=1, conf=None, neighbours=N8,
                window=None):
    """REGION_DTYPE[n] of ``labels[:crop_h, :crop_w]`` from the flood fill: the passing regions
    by (pixels descending, root ascending). ``window`` = (y0, x0, h, w): fill only those cells
    (clipped to the crop); the caller knows that no served pixel lies elsewhere."""
    mask = RG.class_mask(classes)
    y0, x0, y1, x1 = 0, 0, crop_h, crop_w
    if window is not None:
        y0, x0 = window[0], window[1]
        y1, x1 = min(crop_h, y0 + window[2]), min(crop_w, x0 + window[3])
    cf = None if conf is None else np.asarray(conf).tolist()
    rows = []
    for c, px in flood_regions(np.asarray(labels)[y0:y1, x0:x1], mask, neighbours):
        if len(px) < min_pixels:
            continue
        ys = [y0 + p[0] for p in px]
        xs = [x0 + p[1] for p in px]
        sc = 0 if cf is None else sum(cf[y][x] for y, x in zip(ys, xs))
        rows.append((c, ys[0] * crop_w + xs[0], len(px), sum(xs), sum(ys), min(xs), min(ys), max(xs), max(ys),
                     sc, 0, 0))
    rows.sort(key=lambda r: (-r[2], r[1]))
    return np.array(rows, RG.REGION_DTYPE) if rows else np.zeros(0, RG.REGION_DTYPE)


def flood_encode(labels, crop_w, crop_h, classes, min_pixels, K, conf=None, fill=SENT, neighbours=N8,
                 window=None):
    """The frame's row, uint32[4 + 6 K] (7 K with ``conf``), from the flood fill: header, the
    first K records packed, ``fill`` in the words past them."""
    tab = flood_table(labels, crop_w, crop_h, classes, min_pixels, conf, neighbours, window)
    rw = RG.words_per_region(conf is not None)
    out = np.full(4 + rw * K, fill, np.uint32)
    out[:4] = (len(tab), crop_w * crop_h, crop_w, crop_h)
    k = min(len(tab), K)
    out[4:4 + rw * k] = RG.pack(tab[:k], conf is not None).reshape(-1)
    return out


def definition_rows(labels, conf, crop_h, crop_w, classes, min_pixels, K, with_conf):
    """[B, 4 + 6|7 K]: ``regions.encode`` of every frame, SENT in the unwritten words."""
    rw = RG.words_per_region(with_conf)
    return np.stack([RG.encode(l, crop_w, crop_h, classes, min_pixels, K,
                               out=np.full(4 + rw * K, SENT, np.uint32),
                               conf=conf[b] if with_conf else None) for b, l in enumerate(labels)])


# ------------------------------------------------------------------ exhaustive windows
WIN_H, WIN_W = 3, 4
WIN_FILLINGS = 1 << (WIN_H * WIN_W)
WIN_BATCH = 256
WIN_BATCHES = WIN_FILLINGS // WIN_BATCH
WIN_CROP = (TH + 3, TW + 4)                 # (crop_h, crop_w)
WIN_MAP = (WIN_CROP[0] + 2, WIN_CROP[1] + 2)
WIN_CLASSES = (1, 2)
WIN_K = 8
# (row, column) of the window's first cell
WIN_POS = {
    "a": (1, 5),                             # tile interior: rows 1|2 in different waves, 2|3 in one
    "b": (10, TW - 2),                       # across the vertical tile edge
    "c": (TH - 1, 5),                        # across the horizontal tile edge
    "d": (TH - 1, TW - 2),                   # across the four-tile corner
    "e": (WIN_CROP[0] - 2, WIN_CROP[1] - 2), # clipped by the crop's right and bottom edges
}
WIN_PATH = {
    "a": "k_cr_local: run starts and the three union conditions, wave boundary between the rows",
    "b": "k_cr_merge: the left-column lanes (W, NW, SW)",
    "c": "k_cr_merge: the top-row lanes (N, NW, NE)",
    "d": "k_cr_merge: both lane kinds and the diagonals across a tile corner",
    "e": "crop guards: cells outside the crop connect and count nothing",
}


def window_frame(pos, filling):
    """The map of one filling: bit (r * 4 + c) of ``filling`` gives cell (r, c) class 1 or 2;
    unserved class 0 everywhere else. Cells outside the crop are written too."""
    lab = np.zeros(WIN_MAP, np.uint8)
    y0, x0 = WIN_POS[pos]
    for r in range(WIN_H):
        for c in range(WIN_W):
            lab[y0 + r, x0 + c] = 1 + ((filling >> (r * WIN_W + c)) & 1)
    return lab


def window_batch(pos, j):
    """(labels, conf) [256, H, W] of fillings 256 j .. 256 j + 255 at one position."""
    labels = np.stack([window_frame(pos, f) for f in range(j * WIN_BATCH, (j + 1) * WIN_BATCH)])
    rng = np.random.default_rng(1000 * (1 + sorted(WIN_POS).index(pos)) + j)
    conf = rng.integers(0, 256, labels.shape, dtype=np.uint8)
    return labels, conf


_WIN_WANT = {}


def window_want(pos, j, with_conf):
    """[256, 4 + 6|7 K] expected rows of a window batch, from the flood fill on the 12 cells
    (those inside the crop). Built once per (position, batch, form)."""
    key = (pos, j, bool(with_conf))
    if key not in _WIN_WANT:
        labels, conf = window_batch(pos, j)
        ch, cw = WIN_CROP
        win = WIN_POS[pos] + (WIN_H, WIN_W)
        rows = np.stack([flood_encode(l, cw, ch, WIN_CLASSES, 1, WIN_K, conf[b] if with_conf else None,
                                      window=win) for b, l in enumerate(labels)])
        rows.setflags(write=False)
        _WIN_WANT[key] = rows
    return _WIN_WANT[key]


# ------------------------------------------------------------------ builders
@dataclass(frozen=True)
class Built:
    labels: np.ndarray          # [B, H, W] uint8
    conf: np.ndarray            # [B, H, W] uint8
    crop_h: int
    crop_w: int
    classes: Tuple[int, ...]
    min_pixels: int
    K: int

    @property
    def geometry(self):
        return dict(crop_h=self.crop_h, crop_w=self.crop_w, classes=list(self.classes),
                    min_pixels=self.min_pixels, K=self.K)


def least_min_pixels(n):
    """The smallest min_pixels the geometry check accepts for n pixels."""
    return n // (CAND + 1) + 1


def _embed(crops, pad, outside, seed):
    """[B, h + pad[0], w + pad[1]]: the crops top-left, random classes of ``outside`` elsewhere."""
    h, w = crops[0].shape
    rng = np.random.default_rng(seed)
    out = rng.choice(np.asarray(outside, np.uint8), size=(len(crops), h + pad[0], w + pad[1]))
    for i, c in enumerate(crops):
        out[i, :h, :w] = c
    return out


def _built(crops, pad, classes, min_pixels, K, seed, outside=None, conf=None):
    labels = _embed(crops, pad, outside or classes, seed)
    if conf is None:
        conf = np.random.default_rng(seed + 1).integers(0, 256, labels.shape, dtype=np.uint8)
    return Built(labels, np.ascontiguousarray(conf, np.uint8), crops[0].shape[0], crops[0].shape[1],
                 tuple(classes), int(min_pixels), int(K))


# ---- 2. crop shapes
SHAPES = ((1, 1), (1, 7), (7, 1), (1, TW), (TH, 1), (TH - 1, TW - 1), (TH, TW), (TH + 1, TW + 1),
          (2 * TH, 2 * TW), (2 * TH + 1, TW - 1))
SHAPE_SERVED = (1, 2, 3, 4)
SHAPE_UNSERVED = (0, 5)


def blobs(rng, h, w, classes=6, cell=4, noise=0.05):
    coarse = rng.integers(0, classes, (h // cell + 1, w // cell + 1)).astype(np.uint8)
    lab = np.repeat(np.repeat(coarse, cell, 0), cell, 1)[:h, :w].copy()
    sp = rng.random((h, w)) < noise
    lab[sp] = rng.integers(0, classes, int(sp.sum()))
    return lab


def build_shape(h, w):
    rng = np.random.default_rng(31 * h + w)
    blob = blobs(rng, h, w)
    if not np.isin(blob, SHAPE_SERVED).any():
        blob[0, 0] = SHAPE_SERVED[0]
    empty = rng.choice(np.asarray(SHAPE_UNSERVED, np.uint8), size=(h, w))
    return _built([blob, empty], (3, 5), SHAPE_SERVED, least_min_pixels(h * w), 16, 7 * h + w)


def check_shape(b: Built):
    assert (b.crop_h, b.crop_w) in SHAPES and b.labels.shape[2] != b.crop_w
    outside = np.ones(b.labels.shape[1:], bool)
    outside[:b.crop_h, :b.crop_w] = False
    assert np.isin(b.labels[:, outside], b.classes).all()
    n = [len(RG.region_table(l, b.crop_w, b.crop_h, b.classes, b.min_pixels)) for l in b.labels]
    assert n[0] > 0 and n[1] == 0, n
    return {"n_regions": n}


# ---- 3. the coordinate limit
LIMIT = (1 << 16) - 1
LIMIT_SERVED = (3, 7)
LIMIT_UNSERVED = 9


def build_limit(column):
    one = np.full(LIMIT, LIMIT_SERVED[1], np.uint8)
    seg = np.empty(LIMIT, np.uint8)
    at = k = 0
    cycle = LIMIT_SERVED + (LIMIT_UNSERVED,)
    while at < LIMIT:
        seg[at:at + 1 + k % 40] = cycle[k % 3]
        at += 1 + k % 40
        k += 1
    crops = [one[None], seg[None]]
    pad = (1, 2)
    if column:
        crops, pad = [c.T.copy() for c in crops], (2, 2)
    return _built(crops, pad, LIMIT_SERVED, least_min_pixels(LIMIT), KMAX, 65 + column)


def check_limit(b: Built):
    column = b.crop_w == 1
    assert {b.crop_h, b.crop_w} == {1, LIMIT} and LIMIT // b.min_pixels <= CAND < LIMIT // (b.min_pixels - 1)
    RG.check_geometry(b.crop_w, b.crop_h, b.min_pixels, b.K)
    t = RG.region_table(b.labels[0], b.crop_w, b.crop_h, b.classes, b.min_pixels)
    assert len(t) == 1 and t[0]["pixels"] == LIMIT
    hi, s = ("y_max", "sum_y") if column else ("x_max", "sum_x")
    assert t[0][hi] == LIMIT - 1 and t[0][s] == LIMIT * (LIMIT - 1) // 2
    if column:  # the << 16 reaches bit 31
        assert RG.pack(t)[0, 5] >> 31 == 1
    n = len(RG.region_table(b.labels[1], b.crop_w, b.crop_h, b.classes, b.min_pixels))
    assert n > b.K
    return {"min_pixels": b.min_pixels, "n_regions_segments": n}


# ---- 4. selection
SIDE = isqrt(CAND)
SINGLE_CLASSES = (1, 2, 3, 4)


def singletons(h, w):
    """Four classes in a 2 x 2 pattern: no two 8-neighbours share a class."""
    y, x = np.mgrid[:h, :w]
    return (1 + (x & 1) + 2 * (y & 1)).astype(np.uint8)


def build_singletons(keep, K):
    """``keep`` of the SIDE^2 singleton pixels stay; the others turn to the unserved class 0."""
    lab = singletons(SIDE, SIDE)
    if keep < CAND:
        off = np.random.default_rng(keep).permutation(CAND)[keep:]
        lab.reshape(-1)[off] = 0
    return _built([lab], (2, 3), SINGLE_CLASSES, 1, K, 400 + keep + K)


def check_singletons(b: Built, keep):
    assert SIDE * SIDE == CAND and b.crop_h * b.crop_w // b.min_pixels == CAND
    t = RG.region_table(b.labels[0], b.crop_w, b.crop_h, b.classes, b.min_pixels)
    assert len(t) == keep and (t["pixels"] == 1).all()
    return {"candidates": keep}


RECT_CROP = (TH + 9, 2 * TW + 5)
RECT_MIN = 9
RECT_SLOTS = [(2 + 5 * r, 2 + 8 * c) for r in range(RECT_CROP[0] // 5 - 1) for c in range(RECT_CROP[1] // 8)]


def rect_frame(n, big=False):
    """n passing rectangles (3 x 3, every third 3 x 4: area ties) of classes 1 / 2 on unserved
    class 0, scattered over the slots so that raster order is not size order; 2 x 2 decoys
    (below RECT_MIN) in four more slots; ``big``: one 4 x 5 rectangle in another."""
    lab = np.zeros(RECT_CROP, np.uint8)
    order = np.random.default_rng(17).permutation(len(RECT_SLOTS))
    assert n + 5 <= len(order)
    for j in range(n):
        y, x = RECT_SLOTS[order[j]]
        lab[y:y + 3, x:x + 3 + (j % 3 == 2)] = 1 + (j & 1)
    for j in range(n, n + 4):
        y, x = RECT_SLOTS[order[j]]
        lab[y:y + 2, x:x + 2] = 2
    if big:
        y, x = RECT_SLOTS[order[n + 4]]
        lab[y:y + 4, x:x + 5] = 1
    return lab


def build_rects(counts, K, min_pixels=RECT_MIN, big=False):
    return _built([rect_frame(n, big) for n in counts], (3, 4), (1, 2), min_pixels, K, 500 + K + min_pixels)


def check_rects(b: Built, want_counts):
    tabs = [RG.region_table(l, b.crop_w, b.crop_h, b.classes, b.min_pixels) for l in b.labels]
    assert [len(t) for t in tabs] == list(want_counts), [len(t) for t in tabs]
    for t in tabs:  # ties, and inside a tie the roots ascend
        same = t["pixels"][1:] == t["pixels"][:-1]
        assert len(t) < 3 or same.any()
        assert (t["root"][1:][same] > t["root"][:-1][same]).all()
    return {"n_regions": [len(t) for t in tabs], "K": b.K}


def check_threshold(b: Built, equal):
    all_sizes = RG.region_table(b.labels[0], b.crop_w, b.crop_h, b.classes, 1)["pixels"]
    assert ((b.min_pixels if equal else b.min_pixels - 1) == all_sizes).any()
    t = RG.region_table(b.labels[0], b.crop_w, b.crop_h, b.classes, b.min_pixels)
    assert len(t) == int((all_sizes >= b.min_pixels).sum()) and 0 < len(t) < int((all_sizes >= RECT_MIN).sum())
    return {"sizes": sorted(set(all_sizes.tolist())), "min_pixels": b.min_pixels, "n_regions": len(t)}


def build_quota():
    """SIDE x 2 SIDE dominoes at min_pixels 2: N / min_pixels == REGION_CANDIDATES and every
    candidate slot is taken by a region of exactly min_pixels pixels."""
    y, x = np.mgrid[:SIDE, :2 * SIDE]
    lab = (1 + ((x >> 1) & 1) + 2 * (y & 1)).astype(np.uint8)
    return _built([lab], (2, 3), SINGLE_CLASSES, 2, KMAX, 600)


def check_quota(b: Built):
    assert b.crop_h * b.crop_w // b.min_pixels == CAND and b.crop_h * b.crop_w % b.min_pixels == 0
    t = RG.region_table(b.labels[0], b.crop_w, b.crop_h, b.classes, b.min_pixels)
    assert len(t) == CAND and (t["pixels"] == b.min_pixels).all()
    return {"candidates": len(t)}


# ---- 5. statistics slots
STAT_TILES = (4, 5)                                    # tile rows, tile columns
STAT_CROP = (3 * TH + 11, 4 * TW + 7)                  # ragged bottom and right tiles
STAT_MIN = least_min_pixels(STAT_CROP[0] * STAT_CROP[1])


def thin_frame():
    """One 1-pixel path of class 3: a line through every tile row, joined at alternating ends;
    a spur up in tile (0, 3), a spur down in tile (3, 1), the line of tile row 1 alone reaches
    the last column and the line of tile row 2 alone the first."""
    ch, cw = STAT_CROP
    lab = np.zeros(STAT_CROP, np.uint8)
    rows = [r * TH + 9 for r in range(STAT_TILES[0])]
    for y in rows:
        lab[y, 3:cw - 3] = 3
    lab[rows[1], cw - 3:] = 3
    lab[rows[2], :3] = 3
    lab[rows[0]:rows[1], cw - 4] = 3
    lab[rows[1]:rows[2], 3] = 3
    lab[rows[2]:rows[3], cw - 4] = 3
    lab[rows[0] - 1, 3 * TW + 4] = 3
    lab[rows[3] + 1, TW + 4] = 3
    return lab


def _tile_of(y, x):
    return (y // TH, x // TW)


def check_thin(b: Built):
    t, roots = RG.table_and_roots(b.labels[0], b.crop_w, b.crop_h, b.classes, b.min_pixels)
    assert len(t) == 1
    ys, xs = np.divmod(np.flatnonzero(roots == t[0]["root"]), b.crop_w)
    tiles = sorted({_tile_of(y, x) for y, x in zip(ys.tolist(), xs.tolist())})
    ntx = -(-b.crop_w // TW)
    buckets = [(ty * ntx + tx) % BUCKETS for ty, tx in tiles]
    assert len(tiles) > BUCKETS and len(set(buckets)) < len(buckets)
    ext = [{_tile_of(y, x) for y, x in zip(ys[sel].tolist(), xs[sel].tolist())}
           for sel in (xs == xs.min(), xs == xs.max(), ys == ys.min(), ys == ys.max())]
    assert all(len(e) == 1 for e in ext) and len(set.union(*ext)) == 4, ext
    return {"tiles": len(tiles), "extreme_tiles": [sorted(e)[0] for e in ext]}


def reenter_frame():
    """A U of class 2 whose two arms stand in one tile and whose bar lies in the tile below; a
    C of class 1 across a vertical tile edge with a third arm: three pieces in one tile."""
    lab = np.zeros(STAT_CROP, np.uint8)
    lab[TH + 20:2 * TH + 6, TW + 5] = 2
    lab[TH + 20:2 * TH + 6, TW + 15] = 2
    lab[2 * TH + 5, TW + 5:TW + 16] = 2
    for y in (4, 12, 20):
        lab[y, 2 * TW + 20:3 * TW + 4] = 1
    lab[4:21, 3 * TW + 3] = 1
    return lab


def local_pieces(roots2d, root):
    """Most tile-local 8-components of one region in any tile."""
    best = 0
    h, w = roots2d.shape
    for y0 in range(0, h, TH):
        for x0 in range(0, w, TW):
            sub = (roots2d[y0:y0 + TH, x0:x0 + TW] == root).astype(np.uint8)
            best = max(best, len(flood_regions(sub, 2)))
    return best


def check_reenter(b: Built):
    t, roots = RG.table_and_roots(b.labels[0], b.crop_w, b.crop_h, b.classes, b.min_pixels)
    pieces = [local_pieces(roots.reshape(b.crop_h, b.crop_w), int(r)) for r in t["root"]]
    assert sorted(pieces) == [2, 3], pieces
    return {"tile_local_pieces": pieces}


# 256 regions of distinct sizes need sum(m .. m + 255) = 256 m + 32640 pixels: more than the
# 20480 of 5 x 4 tiles, so this one case takes a crop of 9 x 8 tiles (ragged likewise)
SLOTS_CROP = (7 * TH + 11, 8 * TW + 7)
SLOTS_MIN = least_min_pixels(SLOTS_CROP[0] * SLOTS_CROP[1])


def slots_frame():
    """KMAX regions of sizes SLOTS_MIN .. SLOTS_MIN + KMAX - 1 in shuffled order: columns of
    four pixels (the last one shorter) in bands of four rows, an unserved row and column between."""
    ch, cw = SLOTS_CROP
    lab = np.zeros(SLOTS_CROP, np.uint8)
    sizes = SLOTS_MIN + np.random.default_rng(23).permutation(KMAX)
    y = x = 0
    for j, s in enumerate(sizes.tolist()):
        wide = -(-s // 4)
        if x + wide > cw:
            y, x = y + 5, 0
        assert y + 4 <= ch
        c = 1 + (j & 1)
        lab[y:y + 4, x:x + s // 4] = c
        if s % 4:
            lab[y:y + s % 4, x + s // 4] = c
        x += wide + 1
    return lab


def check_slots(b: Built):
    t = RG.region_table(b.labels[0], b.crop_w, b.crop_h, b.classes, b.min_pixels)
    assert len(t) == b.K == KMAX and len(set(t["pixels"].tolist())) == KMAX
    assert t["pixels"].min() == b.min_pixels == SLOTS_MIN
    return {"n_regions": len(t), "sizes": (int(t["pixels"].min()), int(t["pixels"].max()))}


def check_conf_max(b: Built):
    t = RG.region_table(b.labels[0], b.crop_w, b.crop_h, b.classes, b.min_pixels, conf=b.conf[0])
    n = b.crop_h * b.crop_w
    assert len(t) == 1 and t[0]["pixels"] == n and t[0]["sum_conf"] == 255 * n
    return {"sum_conf": 255 * n}


RUN_LINK_STARTS = [3 + 5 * t for t in range(STAT_TILES[1] - 1)]


def runs_frame():
    """Rows of runs of classes 1, 2 (served) and 0, with every (start column in the tile, length)
    pair of a served run that fits a tile row. Rows 0 and 1: in full tile t, class 1 from column
    s to the tile's last column in row 0 and from its first column to s + 2 in row 1; the two
    touch diagonally, so lanes 31 and 32 of the wave hold one key in two rows."""
    ch, cw = STAT_CROP
    rng = np.random.default_rng(41)
    lab = np.zeros(STAT_CROP, np.uint8)
    for t, s in enumerate(RUN_LINK_STARTS):
        lab[0, t * TW + s:(t + 1) * TW] = 1
        lab[1, t * TW:t * TW + s + 3] = 1
    need = {lx: set(range(1, TW - lx + 1)) for lx in range(TW)}
    for y in range(3, ch):
        x, prev = 0, 0
        while x < cw:
            lx = x % TW
            end = lx + min(TW - lx, cw - x)  # of the tile row or the crop, as a tile column
            starts = [s for s in range(lx, end) if any(n <= end - s for n in need[s])]
            c = int(rng.choice([k for k in (1, 2) if k != prev]))
            if starts:  # a pair still missing: mostly the nearest start, class 0 up to it
                s = starts[0] if rng.random() < 0.7 else int(rng.choice(starts))
                x += s - lx
                n = int(rng.choice([n for n in need[s] if n <= end - s]))
                need[s].discard(n)
                if s > lx:
                    c = int(rng.choice((1, 2)))
            else:
                n = int(rng.integers(1, end - lx + 1))
                c = int(rng.choice([k for k in (0, 1, 2) if k != prev or k == 0]))
            lab[y, x:x + n] = c
            x += n
            prev = 0 if x % TW == 0 else c  # a run may go on in the next tile: two runs to the kernel
    return lab


def key_runs(roots2d):
    """{(start column in the tile, length)} of the horizontal runs of one root inside a tile row."""
    out = set()
    h, w = roots2d.shape
    R = roots2d.tolist()
    for y in range(h):
        x = 0
        while x < w:
            r, x1 = R[y][x], x + 1
            while x1 < w and x1 % TW and R[y][x1] == r:
                x1 += 1
            if r >= 0:
                out.add((x % TW, x1 - x))
            x = x1
    return out


def check_runs(b: Built):
    t, roots = RG.table_and_roots(b.labels[0], b.crop_w, b.crop_h, b.classes, b.min_pixels)
    roots = roots.reshape(b.crop_h, b.crop_w)
    runs = key_runs(roots)
    missing = [(lx, n) for lx in range(TW) for n in range(1, TW - lx + 1) if (lx, n) not in runs]
    assert not missing, missing[:10]
    links = 0
    for x0 in range(0, b.crop_w - TW + 1, TW):
        for y in range(0, b.crop_h - 1, 2):  # rows 2 k, 2 k + 1 of a tile: one wave
            if roots[y, x0 + TW - 1] < 0 or roots[y, x0 + TW - 1] != roots[y + 1, x0]:
                continue
            y0 = y - y % TH
            sub = (roots[y0:y0 + TH, x0:x0 + TW] == roots[y, x0 + TW - 1]).astype(np.uint8)
            for _, px in flood_regions(sub, 2):
                links += (y - y0, TW - 1) in px and (y + 1 - y0, 0) in px
    assert links >= len(RUN_LINK_STARTS), links
    return {"run_kinds": len(runs), "lane31_32_links": links, "n_regions": len(t)}


# ------------------------------------------------------------------ the table
@dataclass(frozen=True)
class Case:
    name: str
    path: str                            # the device path the case is there for
    build: Callable[[], Built]
    check: Callable[[Built], dict]       # the predicate, from the reference and the geometry
    forms: Tuple[bool, ...] = (False, True)   # record forms: 6-word, 7-word (with conf)


def _stat(crop_frame, classes, K, seed, conf=None):
    b = _built([crop_frame], (2, 3), classes, STAT_MIN, K, seed)
    if conf is not None:
        b = Built(b.labels, np.full(b.labels.shape, conf, np.uint8), b.crop_h, b.crop_w, b.classes,
                  b.min_pixels, b.K)
    return b


def _cases():
    out = []
    for h, w in SHAPES:
        out.append(Case(f"shape-{h}x{w}", "tile guards of every kernel at thin, exact and ragged crops; n_regions = 0",
                        lambda h=h, w=w: build_shape(h, w), check_shape))
    out += [
        Case("limit-row", "x up to 65534: 16-bit box packing, 32-bit coordinate sum at its bound",
             lambda: build_limit(False), check_limit),
        Case("limit-column", "y up to 65534: y_max << 16 reaches bit 31",
             lambda: build_limit(True), check_limit),
        Case("select-full-K256", "k_cr_select: REGION_CANDIDATES candidates, no padding, every record slot",
             lambda: build_singletons(CAND, KMAX), lambda b: check_singletons(b, CAND)),
        Case("select-full-K1", "k_cr_select: REGION_CANDIDATES candidates, one record",
             lambda: build_singletons(CAND, 1), lambda b: check_singletons(b, CAND)),
        Case("select-4095", "k_cr_select: one padding key",
             lambda: build_singletons(CAND - 1, 64), lambda b: check_singletons(b, CAND - 1)),
        Case("select-1025", "k_cr_select: one candidate more than threads",
             lambda: build_singletons(SELECT_THREADS + 1, KMAX), lambda b: check_singletons(b, SELECT_THREADS + 1)),
        Case("select-0-1-2-3-5-K4", "k_cr_select: sort padded to 2 and 4; n_regions either side of K",
             lambda: build_rects((0, 1, 2, 3, 5), 4), lambda b: check_rects(b, (0, 1, 2, 3, 5))),
        Case("select-7-8-9-K8", "k_cr_select / k_cr_emit: n_regions = K - 1, K, K + 1; ties by root",
             lambda: build_rects((7, 8, 9), 8), lambda b: check_rects(b, (7, 8, 9))),
        Case("select-threshold-equal", "k_cr_gather: cnt == min_pixels passes",
             lambda: build_rects((9,), 16, 12, big=True), lambda b: check_threshold(b, True)),
        Case("select-threshold-above", "k_cr_gather: cnt == min_pixels - 1 does not",
             lambda: build_rects((9,), 16, 13, big=True), lambda b: check_threshold(b, False)),
        Case("select-quota", "k_cr_gather: N / min_pixels == REGION_CANDIDATES, every candidate slot written",
             build_quota, check_quota),
        Case("stats-thin", "k_cr_stats: one slot from 20 tiles, bucket copies shared, box extremes from four tiles",
             lambda: _stat(thin_frame(), (3,), 4, 700), check_thin),
        Case("stats-reenter", "k_cr_stats: two and three tile-local keys of one region in one tile",
             lambda: _stat(reenter_frame(), (1, 2), 4, 710), check_reenter),
        Case("stats-256-slots", "k_cr_select / k_cr_stats / k_cr_emit: every one of the K = 256 slots",
             lambda: _built([slots_frame()], (2, 3), (1, 2), SLOTS_MIN, KMAX, 720), check_slots),
        Case("stats-conf-max", "k_cr_stats<CONF>: the largest sum_conf of the crop",
             lambda: _stat(np.full(STAT_CROP, 5, np.uint8), (5,), 4, 730, conf=255), check_conf_max, forms=(True,)),
        Case("stats-conf-runs", "k_cr_stats<CONF>: segmented shuffle sum, every run start and length",
             lambda: _stat(runs_frame(), (1, 2), KMAX, 740), check_runs, forms=(True,)),
    ]
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

_BUILT = {}
_WANT = {}


def built(case: Case) -> Built:
    """The case's inputs, built once and read-only."""
    if case.name not in _BUILT:
        b = case.build()
        assert b.labels.dtype == np.uint8 and b.conf.shape == b.labels.shape and 1 <= b.K <= KMAX
        RG.check_geometry(b.crop_w, b.crop_h, b.min_pixels, b.K)
        b.labels.setflags(write=False)
        b.conf.setflags(write=False)
        _BUILT[case.name] = b
    return _BUILT[case.name]


def want(case: Case, with_conf: bool) -> np.ndarray:
    """[B, 4 + 6|7 K]: the definition's rows of the case, computed once and read-only."""
    key = (case.name, bool(with_conf))
    if key not in _WANT:
        b = built(case)
        rows = definition_rows(b.labels, b.conf, b.crop_h, b.crop_w, b.classes, b.min_pixels, b.K, with_conf)
        rows.setflags(write=False)
        _WANT[key] = rows
    return _WANT[key]
