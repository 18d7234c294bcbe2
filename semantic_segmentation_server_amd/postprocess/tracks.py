"""Region tracks: the numpy definition of how class regions keep an identity across frames.

``--track_regions`` appends two words to every stored region record (postprocess/regions.py):
``track_id`` and ``age``. Everything is integer; the device kernels (the ``k_tr_*`` chain of
``csrc/hip/class_regions.hip``) and this module agree word for word.

For one stream, take its frames in the order the engine processes them. For frame t:

**Slot plane.** ``S_t[i]``, for the flat crop index ``i = y * crop_w + x``, is the index
(0 .. min(n_regions, K) - 1) of the *stored* region that contains pixel i, in the output order of
``regions.py``. ``S_t[i] = NONE`` (0xFFFF) where the pixel is in no stored region: a class outside
the served set, a region below ``min_pixels``, a region past the first K.

**Overlap.** For stored region a of frame t and stored region b of frame t-1 *with the same
label*, ``O[a][b] = #{ i : S_t[i] == a and S_{t-1}[i] == b }``; pairs of different labels have 0.

**Threshold.** ``--track_min_overlap`` (a float in (0, 1], default 0.25: a choice of the
definition, not a measured value) becomes ``q = round(1024 * ratio)`` once (``quantize``). A pair
is *eligible* iff ``O > 0`` and ``1024 * O >= q * min(pixels_a, pixels_b)``, in 64-bit integers
(O < 2^24, q <= 1024).

**Match** (deterministic, parallel, no sort). ``best[a]``: the eligible b with the largest
``O[a][b]``, ties to the smaller b, none if no b is eligible. ``winner[b]``: among the a with
``best[a] == b`` the one with the largest ``O[a][b]``, ties to the smaller a. a is *matched* iff
``winner[best[a]] == a``. So of the pieces of a split the one with the larger overlap keeps the
id, and a merge takes the id of the predecessor with the larger overlap.

**Ids.** A matched a gets ``track_id = track_id_{t-1}[best[a]]`` and ``age = age_{t-1}[best[a]]
+ 1``. The unmatched stored regions get ``issued + 1, issued + 2, ...`` in slot order with ``age
= 1``; ``issued`` is a per-stream uint32 counter that starts at 0. In a stream's first frame
every region is new. Ids are per stream and per server incarnation.

**Tracking ends** when a region falls out of the first K, drops below ``min_pixels`` or changes
class. There is no re-identification after a gap, no motion model and no use of timestamps:
"previous" is the previously processed frame of the stream.
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import numpy as np

from . import regions as RG

NONE = 0xFFFF
Q_ONE = 1024
DEFAULT_MIN_OVERLAP = 0.25


def quantize(ratio: float) -> int:
    """``q = round(1024 * ratio)`` of a ``--track_min_overlap`` in (0, 1]; ValueError outside."""
    ratio = float(ratio)
    if not 0.0 < ratio <= 1.0:
        raise ValueError(f"--track_min_overlap {ratio} outside (0, 1]")
    return max(1, int(round(Q_ONE * ratio)))


def plane_of(roots: np.ndarray, tab: np.ndarray) -> np.ndarray:
    """uint16[N]: the slot plane from the per-pixel roots (``regions.table_and_roots``) and the
    STORED regions ``tab`` (REGION_DTYPE[<= K], in output order)."""
    roots = np.asarray(roots).reshape(-1)
    plane = np.full(roots.shape, NONE, np.uint16)
    if len(tab):
        slot_of_root = np.full(roots.size, NONE, np.uint16)
        slot_of_root[tab["root"].astype(np.int64)] = np.arange(len(tab), dtype=np.uint16)
        on = roots >= 0
        plane[on] = slot_of_root[roots[on]]
    return plane


def slot_plane(labels: np.ndarray, crop_w: int, crop_h: int, classes, min_pixels: int,
               K: int) -> np.ndarray:
    """uint16[crop_h * crop_w]: per pixel of the crop the index of its stored region, NONE
    where it has none."""
    tab, roots = RG.table_and_roots(labels, crop_w, crop_h, classes, min_pixels)
    return plane_of(roots, tab[:K])


def overlap(cur: np.ndarray, prev: np.ndarray, labels_cur: np.ndarray,
            labels_prev: np.ndarray) -> np.ndarray:
    """int64[n_cur, n_prev]: the pixel overlap of the stored regions of two consecutive frames
    from their slot planes; ``labels_*``: the class of every stored region. Pairs of different
    classes are 0."""
    n, m = len(labels_cur), len(labels_prev)
    cur, prev = np.asarray(cur).reshape(-1), np.asarray(prev).reshape(-1)
    if cur.shape != prev.shape:
        raise ValueError("tracks.overlap: the planes differ in size")
    O = np.zeros((n, m), np.int64)
    if n == 0 or m == 0:
        return O
    both = (cur != NONE) & (prev != NONE)
    key = cur[both].astype(np.int64) * m + prev[both].astype(np.int64)
    O += np.bincount(key, minlength=n * m)[:n * m].reshape(n, m)
    O[np.asarray(labels_cur)[:, None] != np.asarray(labels_prev)[None, :]] = 0
    return O


def associate(O: np.ndarray, pixels_cur: np.ndarray, pixels_prev: np.ndarray,
              q: int) -> Tuple[np.ndarray, np.ndarray]:
    """(best int64[n_cur], matched bool[n_cur]) of an overlap table: ``best[a]`` is -1 where no
    b is eligible."""
    O = np.asarray(O, np.int64)
    n, m = O.shape
    best = np.full(n, -1, np.int64)
    matched = np.zeros(n, bool)
    if n == 0 or m == 0:
        return best, matched
    lo = np.minimum(np.asarray(pixels_cur, np.int64)[:, None], np.asarray(pixels_prev, np.int64)[None, :])
    ok = (O > 0) & (Q_ONE * O >= int(q) * lo)
    Oe = np.where(ok, O, 0)
    b = Oe.argmax(1)  # the first (smallest b) of the largest
    has = ok.any(1)
    best[has] = b[has]
    # winner[b]: of the a whose best is b, the largest overlap, the smaller a on a tie
    claim = np.zeros((n, m), np.int64)
    rows = np.flatnonzero(has)
    claim[rows, best[rows]] = Oe[rows, best[rows]]
    winner = claim.argmax(0)  # the first (smallest a) of the largest
    matched[rows] = winner[best[rows]] == rows
    return best, matched


class StreamTracker:
    """The carried state of one stream: the slot plane, ids, ages, labels and pixel counts of
    its previous frame, and ``issued``."""

    def __init__(self, q: int = quantize(DEFAULT_MIN_OVERLAP)):
        self.q = int(q)
        self.reset()

    def reset(self) -> None:
        """No predecessor, nothing issued: the next frame's regions are all new, from id 1."""
        self.issued = 0
        self.plane: Optional[np.ndarray] = None
        self.prev = np.zeros(0, RG.REGION_DTYPE)

    def update(self, tab: np.ndarray, plane: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
        """Advance by one frame: ``tab`` its STORED regions (REGION_DTYPE[<= K], in order),
        ``plane`` its slot plane -> (track_id uint32[n], age uint32[n])."""
        n = len(tab)
        tid, age = np.zeros(n, np.uint32), np.ones(n, np.uint32)
        best, matched = np.full(n, -1, np.int64), np.zeros(n, bool)
        if self.plane is not None and len(self.prev) and n:
            if self.plane.shape != np.asarray(plane).reshape(-1).shape:
                raise ValueError("tracks: the crop changed inside a stream (reset() first)")
            O = overlap(plane, self.plane, tab["label"], self.prev["label"])
            best, matched = associate(O, tab["pixels"], self.prev["pixels"], self.q)
        tid[matched] = self.prev["track_id"][best[matched]]
        age[matched] = self.prev["age"][best[matched]] + np.uint32(1)
        new = np.flatnonzero(~matched)
        tid[new] = (self.issued + 1 + np.arange(len(new), dtype=np.int64)) & 0xFFFFFFFF
        self.issued = (self.issued + len(new)) & 0xFFFFFFFF
        self.prev = np.array(tab, copy=True)
        self.prev["track_id"], self.prev["age"] = tid, age
        self.plane = np.array(plane, np.uint16, copy=True).reshape(-1)
        return tid, age


class Trackers:
    """One ``StreamTracker`` per stream id, made on first use (the host paths' state)."""

    def __init__(self, q: int):
        self.q = int(q)
        self._by_stream: Dict[int, StreamTracker] = {}

    def of(self, stream: int) -> StreamTracker:
        t = self._by_stream.get(int(stream))
        if t is None:
            t = self._by_stream[int(stream)] = StreamTracker(self.q)
        return t

    def reset(self) -> None:
        self._by_stream = {}


def batch_tables(counts) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """The batch layout of the device kernels from the rows each stream owns
    (``feeder.split_batch``; consecutive rows per stream): int32 (pred[B]: the row of the
    stream's previous frame in the batch, -1: its carried state; stream[B]; last[S]: the last
    row of each stream, -1 for a stream with no row)."""
    counts = [int(c) for c in counts]
    if not counts or min(counts) < 0 or sum(counts) < 1:
        raise ValueError(f"tracks: bad batch layout {counts}")
    pred, stream, last = [], [], []
    for s, c in enumerate(counts):
        for j in range(c):
            pred.append(len(pred) - 1 if j else -1)
            stream.append(s)
        last.append(len(pred) - 1 if c else -1)
    return np.array(pred, np.int32), np.array(stream, np.int32), np.array(last, np.int32)
