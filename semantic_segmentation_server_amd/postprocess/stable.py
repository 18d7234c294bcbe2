"""Stable labels: the numpy definition of the per-pixel temporal debounce of the label maps.

``--stable_labels N`` holds each pixel's label until a different label has been seen for N
consecutive frames of its stream. It runs ahead of everything that reads the label maps (v1
records, masks, class regions, tracks, zone occupancy, zone presence), which all see the
stabilised maps unchanged. Everything is integer; the device kernel (csrc/hip/label_stable.hip)
and this module agree word for word, outputs and state.

For one stream, take its frames in the order the engine processes them. Each pixel ``i = y *
crop_w + x`` of the letterbox-valid crop holds ``(s, c, n, h)``, all uint8: the stable label, the
candidate label, the consecutive frames the candidate has been seen (``0 <= n < N``) and the
held confidence code, with which ``s`` last won. The stream has a ``started`` flag; all zero
means "no predecessor".

Parameters: ``N`` in 2 .. 255 and the confidence gate code ``g`` (``gate_code`` of
``--stable_min_confidence``; 0: no gate). Per pixel a frame brings the raw label ``r`` and the raw
code ``k``; without a confidence plane ``k`` is absent, ``h`` stays 0 and ``g`` must be 0. In this
order:

1. Stream not started: ``s = c = r``, ``n = 0``, ``h = k``; output ``(r, k)``. After the frame
   the stream is started.
2. ``r == s``: ``c = s``, ``n = 0``, ``h = k``; output ``(s, k)``.
3. ``g > 0`` and ``k < g``: a doubtful observation, the state is unchanged; output ``(s, h)``.
4. Otherwise: if ``r == c`` then ``n += 1`` else ``c = r``, ``n = 1``. If ``n >= N`` then ``s = c
   = r``, ``n = 0``, ``h = k`` and the output is ``(r, k)``; else it is ``(s, h)``.

In every case the output is ``(s, h)`` after the update. Pixels of the ``H x W`` plane outside
the crop pass through unchanged and have no state. A stream with no row in a batch keeps its
state. There are no timestamps: "consecutive" counts processed frames of the stream.

The state word of a pixel is ``s | c << 8 | n << 16 | h << 24`` (``pack`` / ``unpack``).
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import numpy as np

MIN_FRAMES, MAX_FRAMES = 2, 255


def gate_code(p: float) -> int:
    """``round(255 * p)`` of a ``--stable_min_confidence`` in [0, 1]; ValueError outside."""
    p = float(p)
    if not 0.0 <= p <= 1.0:
        raise ValueError(f"--stable_min_confidence {p} outside [0, 1]")
    return int(round(255 * p))


def check_params(N: int, g: int, has_conf: bool) -> None:
    """Raise unless ``N`` frames and the gate code ``g`` are a valid pair for label maps with
    (``has_conf``) or without a confidence plane."""
    if not MIN_FRAMES <= int(N) <= MAX_FRAMES:
        raise ValueError(f"--stable_labels {N} outside {MIN_FRAMES} .. {MAX_FRAMES} (0: off)")
    if not 0 <= int(g) <= 255:
        raise ValueError(f"--stable_min_confidence: gate code {g} outside 0 .. 255")
    if int(g) > 0 and not has_conf:
        raise ValueError(f"--stable_min_confidence (gate code {g}) needs the confidence plane "
                         "(--serve_confidence)")


def pack(s, c, n, h) -> np.ndarray:
    """uint32 state words ``s | c << 8 | n << 16 | h << 24``."""
    s, c, n, h = (np.asarray(v).astype(np.uint32) for v in (s, c, n, h))
    return s | c << np.uint32(8) | n << np.uint32(16) | h << np.uint32(24)


def unpack(words) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """(s, c, n, h), uint8 each, of uint32 state words."""
    w = np.asarray(words).astype(np.uint32)
    return tuple(((w >> np.uint32(sh)) & np.uint32(0xFF)).astype(np.uint8) for sh in (0, 8, 16, 24))


class StreamStabilizer:
    """The carried state of one stream: ``started`` and the four uint8 planes over the crop."""

    def __init__(self, N: int, g: int = 0):
        self.N, self.g = int(N), int(g)
        check_params(self.N, self.g, True)
        self.reset()

    def reset(self) -> None:
        """No predecessor: the next frame passes through and becomes the state."""
        self.started = False
        self.crop: Optional[Tuple[int, int]] = None
        self.s = self.c = self.n = self.h = np.zeros(0, np.uint8)

    def state_words(self) -> np.ndarray:
        """uint32[crop_h * crop_w]: the state words (empty before the first frame)."""
        return pack(self.s, self.c, self.n, self.h)

    def step(self, labels_hw, conf_hw, crop_w: int, crop_h: int):
        """Advance by one frame: ``labels_hw`` uint8 [H, W], ``conf_hw`` its confidence codes or
        None -> (stabilised labels, stabilised codes or None), new arrays of the same shapes."""
        lab = np.array(labels_hw, np.uint8, copy=True)
        if lab.ndim != 2 or not (1 <= crop_h <= lab.shape[0] and 1 <= crop_w <= lab.shape[1]):
            raise ValueError(f"stable: crop {crop_w} x {crop_h} outside the map {lab.shape}")
        cf = None
        if conf_hw is not None:
            cf = np.array(conf_hw, np.uint8, copy=True)
            if cf.shape != lab.shape:
                raise ValueError(f"stable: conf {cf.shape} != labels {lab.shape}")
        check_params(self.N, self.g, cf is not None)
        r = lab[:crop_h, :crop_w].reshape(-1)
        k = cf[:crop_h, :crop_w].reshape(-1) if cf is not None else np.zeros(r.shape, np.uint8)
        if not self.started:
            self.crop = (int(crop_w), int(crop_h))
            self.s, self.c, self.h = r.copy(), r.copy(), k.copy()
            self.n = np.zeros(r.shape, np.uint8)
            self.started = True
        else:
            if self.crop != (int(crop_w), int(crop_h)):
                raise ValueError("stable: the crop changed inside a stream (reset() first)")
            s, c, n, h = self.s, self.c, self.n.astype(np.int32), self.h
            same = r == s
            act = ~same if self.g == 0 else ~same & (k >= self.g)  # rule 4; the rest of ~same: rule 3
            n = np.where(act, np.where(r == c, n + 1, 1), np.where(same, 0, n))
            c = np.where(act, r, np.where(same, s, c))
            win = act & (n >= self.N)
            s = np.where(win, r, s)
            n = np.where(win, 0, n)
            h = np.where(same | win, k, h)
            self.s, self.c, self.n, self.h = (v.astype(np.uint8) for v in (s, c, n, h))
        lab[:crop_h, :crop_w] = self.s.reshape(crop_h, crop_w)
        if cf is not None:
            cf[:crop_h, :crop_w] = self.h.reshape(crop_h, crop_w)
        return lab, cf


class Stabilizers:
    """One ``StreamStabilizer`` per stream id, made on first use (the host paths' state)."""

    def __init__(self, N: int, g: int = 0):
        self.N, self.g = int(N), int(g)
        check_params(self.N, self.g, True)
        self._by_stream: Dict[int, StreamStabilizer] = {}

    def of(self, stream: int) -> StreamStabilizer:
        t = self._by_stream.get(int(stream))
        if t is None:
            t = self._by_stream[int(stream)] = StreamStabilizer(self.N, self.g)
        return t

    def step(self, labels, conf, crop_w: int, crop_h: int, streams):
        """A batch: ``labels`` uint8 [B, H, W], ``conf`` the same or None, ``streams`` the stream
        id of every row, taken in row order -> (labels, conf) stabilised, new arrays."""
        labels = np.asarray(labels, np.uint8)
        out = np.empty_like(labels)
        cout = None if conf is None else np.empty_like(labels)
        if len(streams) != labels.shape[0]:
            raise ValueError(f"stable: {len(streams)} streams for {labels.shape[0]} frames")
        for b, st in enumerate(streams):
            lb, cb = self.of(st).step(labels[b], None if conf is None else np.asarray(conf)[b],
                                      crop_w, crop_h)
            out[b] = lb
            if cout is not None:
                cout[b] = cb
        return out, cout

    def reset(self) -> None:
        self._by_stream = {}


def batch_tables(counts) -> np.ndarray:
    """The batch layout of the device kernel from the rows each stream owns
    (``feeder.split_batch``; consecutive rows per stream): int32 [first[S] | count[S]]."""
    counts = [int(c) for c in counts]
    if not counts or min(counts) < 0 or sum(counts) < 1:
        raise ValueError(f"stable: bad batch layout {counts}")
    first = np.concatenate([[0], np.cumsum(counts)[:-1]])
    return np.concatenate([first, counts]).astype(np.int32)
