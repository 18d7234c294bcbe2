"""Zone presence: per frame, the exact pixel overlap of every stored class region with every
zone, and with region tracks how long each track has been inside each zone (``--serve_presence``,
v2 GetZonePresence). This file is the one definition: the oracle of the device kernels
(csrc/hip/zone_presence.hip), the implementation of the CPU / ``--backend torch`` / host
post-processing paths, and the decoder behind the RPC. Everything is integer.

For one frame, ``S[i]`` is the slot plane of postprocess/tracks.py (the index of the stored
region that holds crop pixel ``i``, ``0xFFFF`` for none), ``n = min(n_regions, K)`` the number
of stored regions, ``plane`` the zone plane of postprocess/zones.py and ``R = 1 + Z`` the number
of zone rows (row 0: the whole crop).

**Counts.** ``P[a][0] = #{i : S[i] == a}`` (the region's ``pixels``) and, for ``r = 1 .. Z``,
``P[a][r] = #{i : S[i] == a and bit r - 1 of plane[i]}``.

**Inside.** ``--presence_min_share`` (a float in (0, 1], default 0.5: a choice of the definition,
not a measured value) becomes ``q = max(1, round(1024 * share))`` once (``quantize``). Region a is
*inside* row r iff ``P[a][r] > 0`` and ``1024 * P[a][r] >= q * pixels_a`` in 64-bit integers;
row 0 is always inside.

**Dwell** (with ``--track_regions``). ``D[a][r] = (D_prev[pred(a)][r] if a is matched else 0)
+ 1`` if a is inside r, else 0, in uint32 like ``age``. ``pred(a)`` is ``best[a]`` of a matched
region in tracks.py: the region of the stream's previous frame whose ``track_id`` a keeps. (A
region is matched iff its ``age > 1``, and the ids of one frame are distinct, so the host state
is keyed by ``track_id``; the device reads the link table of the tracking kernels.) Hence
``D[a][0] == age``; a track that leaves a zone drops to 0 and restarts at 1 when it re-enters;
of the pieces of a split the one that keeps the id inherits the dwell. Dwell counts processed
frames of the stream, not seconds.

**Words.** A frame is ``uint32[4 + U K]``: the header ``n, N, crop_w, crop_h``, then for each
stored region ``a < n`` the entry ``(label << 24) | root`` (the region record's first word),
``track_id`` (0 without tracks), ``P[a][0 .. R - 1]`` and, with tracks, ``D[a][0 .. R - 1]``:
``U = 2 + R``, or ``2 + 2 R`` with tracks. Every word is written every time, zeros past entry n.

**Limits** (``check_geometry``): ``N < 2^24``, ``Z <= 32``, ``1 <= K <= 256`` (the kernel's
on-chip table holds ``K x R <= 256 x 33`` counters).
"""
from __future__ import annotations

from typing import Dict, NamedTuple, Optional

import numpy as np

from . import regions as RG
from . import tracks as TK
from . import zones as ZN

HEADER = 4
Q_ONE = 1024
DEFAULT_MIN_SHARE = 0.5
MAX_ZONES = ZN.MAX_ZONES
MAX_REGIONS = RG.MAX_REGIONS
MAX_PIXELS = 1 << 24
NONE = TK.NONE


def quantize(share: float) -> int:
    """``q = max(1, round(1024 * share))`` of a ``--presence_min_share`` in (0, 1]."""
    share = float(share)
    if not 0.0 < share <= 1.0:
        raise ValueError(f"--presence_min_share {share} outside (0, 1]")
    return max(1, int(round(Q_ONE * share)))


def unit(rows: int, tracks: bool = False) -> int:
    """U: the words of one entry."""
    return 2 + int(rows) * (2 if tracks else 1)


def frame_words(K: int, rows: int, tracks: bool = False) -> int:
    return HEADER + unit(rows, tracks) * int(K)


def check_geometry(crop_w: int, crop_h: int, num_zones: int, K: int) -> None:
    """Raise unless ``--serve_presence`` can serve ``K`` regions against ``num_zones`` user zones
    in a ``crop_w x crop_h`` crop."""
    if crop_w < 1 or crop_h < 1:
        raise ValueError(f"--serve_presence: empty crop {crop_w} x {crop_h}")
    if crop_w * crop_h >= MAX_PIXELS:
        raise ValueError(f"--serve_presence: {crop_w} x {crop_h} = {crop_w * crop_h} pixels; a "
                         f"region root needs fewer than 2^24 = {MAX_PIXELS} (lower --input_size)")
    if not 0 <= num_zones <= MAX_ZONES:
        raise ValueError(f"--serve_presence: {num_zones} zones, at most {MAX_ZONES} (--zones)")
    if not 1 <= K <= MAX_REGIONS:
        raise ValueError(f"--serve_presence: --max_regions {K} outside 1 .. {MAX_REGIONS}")


def counts(slots: np.ndarray, plane: Optional[np.ndarray], n: int, rows: int) -> np.ndarray:
    """uint32 [n, R]: ``P`` of a slot plane (uint16 [N]) against the zone plane (uint32 [N] or
    [crop_h, crop_w]; None: row 0 alone)."""
    S = np.asarray(slots).reshape(-1).astype(np.int64)
    P = np.zeros((n, rows), np.uint32)
    if n == 0:
        return P
    on = S < n
    P[:, 0] = np.bincount(S[on], minlength=n)[:n]
    if rows > 1:
        pl = np.asarray(plane).reshape(-1).astype(np.uint32)
        if pl.shape != S.shape:
            raise ValueError(f"presence: the zone plane has {pl.size} pixels, the slot plane {S.size}")
        for r in range(1, rows):
            sel = on & ((pl >> np.uint32(r - 1)) & np.uint32(1)).astype(bool)
            P[:, r] = np.bincount(S[sel], minlength=n)[:n]
    return P


def inside(P: np.ndarray, q: int) -> np.ndarray:
    """bool [n, R] of the counts ``P`` (column 0: the regions' pixels)."""
    P = np.asarray(P).astype(np.int64)
    if P.ndim != 2 or P.shape[1] < 1:
        raise ValueError("presence.inside: P must be [n, R]")
    ins = (P > 0) & (Q_ONE * P >= int(q) * P[:, :1])
    ins[:, 0] = True
    return ins


class StreamDwell:
    """The carried dwell state of one stream: the ``track_id`` and the ``D`` row of every
    stored region of its previous frame."""

    def __init__(self):
        self.reset()

    def reset(self) -> None:
        self.ids = np.zeros(0, np.uint32)
        self.D = np.zeros((0, 1), np.uint32)

    def update(self, track_id: np.ndarray, age: np.ndarray, ins: np.ndarray) -> np.ndarray:
        """Advance by one frame -> uint32 [n, R]."""
        n, R = ins.shape
        prev = np.zeros((n, R), np.uint32)
        if len(self.ids) and n and self.D.shape[1] == R:
            at = {int(t): k for k, t in enumerate(self.ids)}
            for a in range(n):
                k = at.get(int(track_id[a])) if int(age[a]) > 1 else None
                if k is not None:
                    prev[a] = self.D[k]
        D = np.where(ins, prev + np.uint32(1), np.uint32(0)).astype(np.uint32)
        self.ids, self.D = np.array(track_id, np.uint32, copy=True), D
        return D


class Dwells:
    """One ``StreamDwell`` per stream id, made on first use (the host paths' state)."""

    def __init__(self):
        self._by_stream: Dict[int, StreamDwell] = {}

    def of(self, stream: int) -> StreamDwell:
        d = self._by_stream.get(int(stream))
        if d is None:
            d = self._by_stream[int(stream)] = StreamDwell()
        return d

    def reset(self) -> None:
        self._by_stream = {}


def encode_slots(slots: np.ndarray, tab: np.ndarray, plane: Optional[np.ndarray], crop_w: int,
                 crop_h: int, K: int, rows: int, q: int, dwell: Optional[StreamDwell] = None,
                 out: Optional[np.ndarray] = None) -> np.ndarray:
    """The frame words from the slot plane ``slots`` (uint16 [N]) and the STORED regions ``tab``
    (REGION_DTYPE[<= K], in order; with ``dwell`` their ``track_id`` and ``age`` are read).
    ``dwell``: the state of this frame's stream, advanced by this call."""
    R, K, n = int(rows), int(K), len(tab)
    check_geometry(crop_w, crop_h, R - 1, K)
    if n > K:
        raise ValueError(f"presence: {n} stored regions, K = {K}")
    if plane is None and R != 1:
        raise ValueError(f"presence: {R} rows need a zone plane")
    tr = dwell is not None
    U, nw = unit(R, tr), frame_words(K, R, tr)
    if out is None:
        out = np.zeros(nw, np.uint32)
    elif out.shape != (nw,) or out.dtype != np.uint32:
        raise ValueError(f"presence: out must be uint32[{nw}]")
    out[:] = 0
    out[:HEADER] = (n, crop_w * crop_h, crop_w, crop_h)
    P = counts(slots, plane, n, R)
    e = out[HEADER:HEADER + U * n].reshape(n, U)
    e[:, 0] = (tab["label"].astype(np.uint32) << 24) | tab["root"]
    e[:, 2:2 + R] = P
    if tr:
        e[:, 1] = tab["track_id"]
        e[:, 2 + R:] = dwell.update(tab["track_id"], tab["age"], inside(P, q))
    return out


def encode(labels: np.ndarray, plane: Optional[np.ndarray], crop_w: int, crop_h: int, classes,
           min_pixels: int, K: int, rows: int, q: int, tab: Optional[np.ndarray] = None,
           dwell: Optional[StreamDwell] = None, out: Optional[np.ndarray] = None) -> np.ndarray:
    """The frame words of one label map (uint8 [H, W], read inside the crop). ``tab``: with
    ``dwell``, the frame's stored regions with their ``track_id`` and ``age`` (``regions.decode``
    of the frame's region words); they must be the regions of ``labels``."""
    full, roots = RG.table_and_roots(labels, crop_w, crop_h, classes, min_pixels)
    mine = full[:K]
    if dwell is not None:
        if tab is None or len(tab) != len(mine) or not np.array_equal(tab["root"], mine["root"]):
            raise ValueError("presence.encode: tab does not hold the stored regions of labels")
        mine = np.array(mine, copy=True)
        mine["track_id"], mine["age"] = tab["track_id"], tab["age"]
    return encode_slots(TK.plane_of(roots, mine), mine, plane, crop_w, crop_h, K, rows, q, dwell, out)


class Presence(NamedTuple):
    n: int                  # stored regions
    pixels_total: int       # N = crop_w * crop_h
    crop_w: int
    crop_h: int
    label: np.ndarray       # uint8 [n]
    root: np.ndarray        # uint32 [n]
    track_id: np.ndarray    # uint32 [n]; 0 without tracks
    P: np.ndarray           # uint32 [n, R]
    D: Optional[np.ndarray]  # uint32 [n, R], or None without tracks


def used_words(words: np.ndarray, rows: int, tracks: bool = False) -> int:
    """Header + entries: ``4 + U n``."""
    return HEADER + unit(rows, tracks) * int(words[0])


def decode(words: np.ndarray, rows: int, tracks: bool = False) -> Presence:
    """One frame's words (at least the used ones) -> its entries."""
    w = np.asarray(words)
    if w.dtype != np.uint32:
        w = w.view(np.uint32)
    if w.ndim != 1 or len(w) < HEADER:
        raise ValueError("presence.decode: expected one frame's uint32 words")
    R, U = int(rows), unit(rows, tracks)
    n, N, cw, ch = (int(v) for v in w[:HEADER])
    if N != cw * ch or N < 1 or N >= MAX_PIXELS or n > MAX_REGIONS or len(w) < HEADER + U * n:
        raise ValueError(f"presence.decode: bad header (entries {n}, N {N}, crop {cw} x {ch}) or "
                         f"{len(w)} words do not hold {n} entries of {U}")
    e = w[HEADER:HEADER + U * n].reshape(n, U)
    return Presence(n, N, cw, ch, (e[:, 0] >> np.uint32(24)).astype(np.uint8),
                    e[:, 0] & np.uint32(0xFFFFFF), e[:, 1].copy(), e[:, 2:2 + R],
                    e[:, 2 + R:2 + 2 * R] if tracks else None)
