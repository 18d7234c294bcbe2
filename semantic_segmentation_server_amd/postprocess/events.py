"""Zone events: the edges of the zone-presence state between two consecutive processed frames
of a stream -- a track entered a zone, a track left it after n frames, a track was born, a track
ended (``--serve_events``, v2 GetZoneEvents). This file is the one definition: the oracle of the
device kernels (csrc/hip/zone_events.hip), the implementation of the CPU / ``--backend torch`` /
host post-processing paths, and the decoder behind the RPC. Everything is integer.

``prev`` and ``cur`` are the decoded presence rows with tracks (postprocess/presence.py) of two
consecutive processed frames of one stream: ``n`` stored entries with ``first = (label << 24) |
root``, ``track_id``, ``P[n][R]`` and ``D[n][R]``. Before a stream's first frame, and after a
reset, ``prev`` has ``n = 0``.

**Successor.** ``succ(b)`` is the entry a of ``cur`` with ``cur.track_id[a] == prev.track_id[b]``,
or none. The ids of one frame are distinct and non-zero and a fresh id is never reused
(postprocess/tracks.py), so it is well defined.

**LEAVE** ``(b, r)``, ``b < prev.n``, ``r < R``: ``prev.D[b][r] > 0`` and (``succ(b)`` is none or
``cur.D[succ(b)][r] == 0``). **ENTER** ``(a, r)``, ``a < cur.n``: ``cur.D[a][r] == 1``. Row 0 is
the whole crop: its ENTER is the track's birth, its LEAVE the track's end. The definition is
total over any pair of rows whose ids are distinct and non-zero within each frame; it does not
assume that ``D`` is dwell-consistent.

**Order.** All LEAVEs ascending in ``(b, r)``, then all ENTERs ascending in ``(a, r)``.

**An event** is 4 words: ``w0 = slot | r << 8 | kind << 16 | edge << 24`` (slot: a or b, below
256; kind 1 ENTER, 2 LEAVE; edge 1 iff the track itself begins -- ``cur.D[a][0] == 1`` -- or ends
-- ``succ(b)`` is none -- here), ``w1 = track_id``, ``w2 = first`` of the entry, ``w3 =
cur.P[a][r]`` (ENTER: the pixels inside at entry) or ``prev.D[b][r]`` (LEAVE: the frames it stayed).

**A frame** is ``uint32[4 + 4 E]``: the header ``n_events`` (the true total), ``N``, ``crop_w``,
``crop_h``, then the first ``min(n_events, E)`` events; zeros fill the rest. ``E`` is
``--max_events`` (``check_geometry``: 1 .. 4096).
"""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np

from . import presence as PR

HEADER = 4
EVENT_WORDS = 4
ENTER, LEAVE = 1, 2
DEFAULT_MAX_EVENTS = 64
MAX_EVENTS = 4096
DEFAULT_EVENT_LOG = 4096

DECODED_DTYPE = np.dtype([("slot", np.uint8), ("zone", np.uint8), ("kind", np.uint8),
                          ("edge", np.uint8), ("track_id", np.uint32), ("label", np.uint8),
                          ("root", np.uint32), ("value", np.uint32)])


def check_geometry(max_events: int) -> None:
    """Raise unless ``--max_events`` is a capacity the kernels serve."""
    if not 1 <= int(max_events) <= MAX_EVENTS:
        raise ValueError(f"--serve_events: --max_events {max_events} outside 1 .. {MAX_EVENTS}")


def frame_words(E: int) -> int:
    return HEADER + EVENT_WORDS * int(E)


def used_words(words: np.ndarray) -> int:
    """Header + stored events: ``4 + 4 min(n_events, E)`` of one frame's full row."""
    E = (len(words) - HEADER) // EVENT_WORDS
    return HEADER + EVENT_WORDS * min(int(words[0]), E)


_EMPTY = PR.Presence(0, 0, 0, 0, np.zeros(0, np.uint8), np.zeros(0, np.uint32),
                     np.zeros(0, np.uint32), np.zeros((0, 1), np.uint32), np.zeros((0, 1), np.uint32))


def between(prev: Optional[PR.Presence], cur: PR.Presence, E: int,
            out: Optional[np.ndarray] = None) -> np.ndarray:
    """The frame words of the events from ``prev`` (None: no predecessor) to ``cur``."""
    check_geometry(E)
    nw = frame_words(E)
    if out is None:
        out = np.zeros(nw, np.uint32)
    elif out.shape != (nw,) or out.dtype != np.uint32:
        raise ValueError(f"events: out must be uint32[{nw}]")
    out[:] = 0
    if cur.D is None:
        raise ValueError("events: the presence rows carry no dwell (--track_regions)")
    R = cur.P.shape[1]
    if prev is None or prev.n == 0:
        prev = _EMPTY
    elif prev.D is None or prev.D.shape[1] != R:
        raise ValueError("events: prev and cur differ in their zone rows")
    cur_first = (cur.label.astype(np.uint32) << np.uint32(24)) | cur.root
    prev_first = (prev.label.astype(np.uint32) << np.uint32(24)) | prev.root
    # succ, and per LEAVE candidate the dwell of its successor (0 without one)
    at = {int(t): a for a, t in enumerate(cur.track_id)}
    succ = np.array([at.get(int(t), -1) for t in prev.track_id], np.int64).reshape(-1)
    after = np.zeros((prev.n, R), np.uint32)
    has = succ >= 0
    if has.any():
        after[has] = cur.D[succ[has]]
    pD = prev.D if prev.n else np.zeros((0, R), np.uint32)
    lb, lr = np.nonzero((pD > 0) & (after == 0))      # row-major: ascending (b, r)
    ea, er = np.nonzero(cur.D == 1)
    nl, ne = len(lb), len(ea)
    ev = np.zeros((nl + ne, EVENT_WORDS), np.uint32)
    ev[:nl, 0] = (lb | (lr << 8) | (LEAVE << 16) | ((~has[lb]).astype(np.int64) << 24)).astype(np.uint32)
    ev[:nl, 1] = prev.track_id[lb]
    ev[:nl, 2] = prev_first[lb]
    ev[:nl, 3] = pD[lb, lr]
    ev[nl:, 0] = (ea | (er << 8) | (ENTER << 16)
                  | ((cur.D[ea, 0] == 1).astype(np.int64) << 24)).astype(np.uint32)
    ev[nl:, 1] = cur.track_id[ea]
    ev[nl:, 2] = cur_first[ea]
    ev[nl:, 3] = cur.P[ea, er]
    out[:HEADER] = (nl + ne, cur.pixels_total, cur.crop_w, cur.crop_h)
    k = min(nl + ne, int(E))
    out[HEADER:HEADER + EVENT_WORDS * k] = ev[:k].reshape(-1)
    return out


def events_between(prev_words: Optional[np.ndarray], cur_words: np.ndarray, R: int, E: int,
                   out: Optional[np.ndarray] = None) -> np.ndarray:
    """``between`` on raw presence words with tracks (``prev_words`` None or with ``n = 0``: no
    predecessor)."""
    prev = None
    if prev_words is not None and int(np.asarray(prev_words).view(np.uint32)[0]):
        prev = PR.decode(prev_words, R, tracks=True)
    return between(prev, PR.decode(cur_words, R, tracks=True), E, out)


def _own(p: PR.Presence) -> PR.Presence:
    return PR.Presence(p.n, p.pixels_total, p.crop_w, p.crop_h, *(np.array(v, copy=True) for v in p[4:]))


class StreamEvents:
    """The carried state of one stream: its previous decoded presence row."""

    def __init__(self, E: int = DEFAULT_MAX_EVENTS):
        check_geometry(E)
        self.E = int(E)
        self.reset()

    def reset(self) -> None:
        self.prev: Optional[PR.Presence] = None

    def update(self, cur: PR.Presence, out: Optional[np.ndarray] = None) -> np.ndarray:
        """Advance by one frame -> its event words."""
        words = between(self.prev, cur, self.E, out)
        self.prev = _own(cur)
        return words


class Events:
    """One ``StreamEvents`` per stream id, made on first use (the host paths' state)."""

    def __init__(self, E: int = DEFAULT_MAX_EVENTS):
        check_geometry(E)
        self.E = int(E)
        self._by_stream: Dict[int, StreamEvents] = {}

    def of(self, stream: int) -> StreamEvents:
        s = self._by_stream.get(int(stream))
        if s is None:
            s = self._by_stream[int(stream)] = StreamEvents(self.E)
        return s

    def reset(self) -> None:
        self._by_stream = {}


def decode(words: np.ndarray) -> np.ndarray:
    """One frame's words (at least the used ones), or bare ``[n, 4]`` event words -> DECODED_DTYPE
    [stored events]; ``value`` is ``pixels`` of an ENTER and ``dwell`` of a LEAVE."""
    w = np.asarray(words)
    if w.dtype != np.uint32:
        w = w.view(np.uint32)
    if w.ndim == 1:
        if len(w) < HEADER:
            raise ValueError("events.decode: expected one frame's uint32 words")
        k = min(int(w[0]), (len(w) - HEADER) // EVENT_WORDS)
        w = w[HEADER:HEADER + EVENT_WORDS * k].reshape(k, EVENT_WORDS)
    elif w.ndim != 2 or w.shape[1] != EVENT_WORDS:
        raise ValueError("events.decode: expected [n, 4] event words")
    ev = np.zeros(len(w), DECODED_DTYPE)
    ev["slot"], ev["zone"] = w[:, 0] & 0xFF, (w[:, 0] >> 8) & 0xFF
    ev["kind"], ev["edge"] = (w[:, 0] >> 16) & 0xFF, (w[:, 0] >> 24) & 0xFF
    ev["track_id"], ev["label"], ev["root"] = w[:, 1], w[:, 2] >> 24, w[:, 2] & 0xFFFFFF
    ev["value"] = w[:, 3]
    return ev
