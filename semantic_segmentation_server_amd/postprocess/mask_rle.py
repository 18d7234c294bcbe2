"""Run-length encoding of label masks: the numpy definition of the format.

A frame's mask is the letterbox-valid region ``labels[:crop_h, :crop_w]`` of the
model-resolution label map, read as ONE flat row-major sequence of ``N = crop_h * crop_w``
pixels (flat index ``i = y * crop_w + x``: runs continue across row ends). Pixel ``i``
starts a run iff ``i == 0`` or ``L(i) != L(i - 1)``.

Per frame, on the device and on the host, ``uint32[4 + cap]``::

    word 0      n_runs, the true total (may exceed cap)
    word 1      N
    word 2      crop_w
    word 3      crop_h
    word 4 + k  (label << 24) | start_k    for k < min(n_runs, cap), in run order

Words past ``4 + min(n_runs, cap)`` are not written. Starts are stored, not lengths (the
device kernel needs no look-ahead); lengths are differences, taken where an RPC asks for
them (``to_wire``). ``N < 2**24`` so a start fits 24 bits. If ``n_runs > cap`` the mask is
*truncated*: the first ``cap - 1`` runs are kept (the last stored run's length is then
known from the next stored start).

This module is the oracle of the device encoder (``csrc/hip/mask_rle.hip``), the encoder of
the CPU / torch paths, and the decoder of the client.
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np

HEADER = 4
MAX_PIXELS = 1 << 24
UNCOVERED = 255  # decode(allow_truncated=True): pixels past the last kept run


def check_geometry(crop_w: int, crop_h: int, cap: int) -> None:
    """Raise ValueError unless a ``crop_h x crop_w`` mask with ``cap`` run slots is encodable."""
    if crop_w < 1 or crop_h < 1:
        raise ValueError(f"mask_rle: empty crop {crop_h} x {crop_w}")
    if crop_w * crop_h >= MAX_PIXELS:
        raise ValueError(f"mask_rle: {crop_h} x {crop_w} = {crop_w * crop_h} pixels do not fit "
                         f"24-bit run starts (N < {MAX_PIXELS} required)")
    if cap < 2:
        raise ValueError(f"mask_rle: cap {cap} < 2")


def encode(labels: np.ndarray, crop_w: int, crop_h: int, cap: int,
           out: Optional[np.ndarray] = None) -> np.ndarray:
    """``labels[H, W]`` uint8 -> ``uint32[4 + cap]``. Unwritten words keep ``out``'s values
    (zero without ``out``)."""
    labels = np.asarray(labels)
    if labels.ndim != 2 or labels.dtype != np.uint8:
        raise ValueError("mask_rle.encode: labels must be a 2-D uint8 map")
    check_geometry(crop_w, crop_h, cap)
    if crop_h > labels.shape[0] or crop_w > labels.shape[1]:
        raise ValueError(f"mask_rle.encode: crop {crop_h} x {crop_w} outside the "
                         f"{labels.shape[0]} x {labels.shape[1]} map")
    if out is None:
        out = np.zeros(HEADER + cap, np.uint32)
    elif out.shape != (HEADER + cap,) or out.dtype != np.uint32:
        raise ValueError("mask_rle.encode: out must be uint32[4 + cap]")
    flat = labels[:crop_h, :crop_w].reshape(-1)
    n = flat.size
    starts = np.flatnonzero(np.concatenate(([True], flat[1:] != flat[:-1])))
    k = min(len(starts), cap)
    out[0], out[1], out[2], out[3] = len(starts), n, crop_w, crop_h
    out[HEADER:HEADER + k] = (flat[starts[:k]].astype(np.uint32) << 24) | starts[:k].astype(np.uint32)
    return out


def used_words(words: np.ndarray, cap: Optional[int] = None) -> int:
    """Header + stored runs: ``4 + min(n_runs, cap)`` (``cap`` defaults to the array's)."""
    cap = len(words) - HEADER if cap is None else cap
    return HEADER + min(int(words[0]), cap)


def _runs(words: np.ndarray) -> Tuple[np.ndarray, np.ndarray, np.ndarray, bool, int, int, int]:
    """(labels, starts, lengths, truncated, total_runs, crop_w, crop_h) of the kept runs."""
    words = np.asarray(words)
    if words.ndim != 1 or len(words) < HEADER:
        raise ValueError("mask_rle: words must be a 1-D array with the 4 header words")
    words = words.view(np.uint32) if words.dtype == np.int32 else words.astype(np.uint32, copy=False)
    total, n, cw, ch = (int(v) for v in words[:HEADER])
    if n != cw * ch or n < 1 or n >= MAX_PIXELS or total < 1 or total > n:
        raise ValueError(f"mask_rle: bad header (runs {total}, N {n}, crop {ch} x {cw})")
    stored = min(total, len(words) - HEADER)
    truncated = stored < total
    if truncated and stored < 2:
        raise ValueError("mask_rle: a truncated mask needs at least two stored runs")
    ent = words[HEADER:HEADER + stored]
    starts = (ent & np.uint32(0xFFFFFF)).astype(np.int64)
    if starts[0] != 0 or (np.diff(starts) <= 0).any() or starts[-1] >= n:
        raise ValueError("mask_rle: run starts are not strictly increasing from 0")
    ends = np.concatenate((starts[1:], [n]))
    keep = stored - 1 if truncated else stored
    return ((ent[:keep] >> np.uint32(24)).astype(np.uint8), starts[:keep],
            (ends - starts)[:keep].astype(np.uint32), truncated, total, cw, ch)


def decode(words: np.ndarray, allow_truncated: bool = False) -> np.ndarray:
    """``uint32[>= 4 + min(n_runs, cap)]`` -> ``uint8[crop_h, crop_w]``. A truncated mask raises
    unless ``allow_truncated``; its uncovered pixels are then 255."""
    labs, starts, lens, truncated, total, cw, ch = _runs(words)
    if truncated and not allow_truncated:
        raise ValueError(f"mask_rle.decode: mask truncated ({len(labs)} of {total} runs kept)")
    flat = np.full(cw * ch, UNCOVERED, np.uint8)
    covered = int(lens.sum())
    flat[:covered] = np.repeat(labs, lens)
    return flat.reshape(ch, cw)


def to_wire(words: np.ndarray) -> Tuple[bytes, np.ndarray, bool, int]:
    """(run_labels: one class id byte per run, run_lengths uint32[], truncated, total_runs).
    The lengths sum to ``crop_w * crop_h`` unless truncated (then to the start of the first
    dropped run)."""
    labs, _, lens, truncated, total, _, _ = _runs(words)
    return labs.tobytes(), lens, truncated, total


def from_wire(run_labels: bytes, run_lengths, width: int, height: int,
              allow_truncated: bool = False) -> np.ndarray:
    """The client's decoder: wire runs -> ``uint8[height, width]`` (uncovered pixels 255)."""
    labs = np.frombuffer(run_labels, np.uint8)
    lens = np.asarray(run_lengths, np.int64)
    if len(labs) != len(lens) or (lens <= 0).any():
        raise ValueError("mask_rle.from_wire: one positive length per run label required")
    covered = int(lens.sum())
    if covered > width * height or (covered < width * height and not allow_truncated):
        raise ValueError(f"mask_rle.from_wire: runs cover {covered} of {width * height} pixels")
    flat = np.full(width * height, UNCOVERED, np.uint8)
    flat[:covered] = np.repeat(labs, lens)
    return flat.reshape(height, width)
