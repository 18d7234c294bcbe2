"""Smooth labels: the numpy definition of the windowed majority filter of the label maps.

``--smooth_labels R`` replaces every pixel's label by the most frequent label of its (2R+1) x
(2R+1) window. It runs ahead of everything that reads the label maps, the temporal
stabilisation (``--stable_labels``) included, which all see the smoothed maps unchanged.
Everything is integer; the device kernel (csrc/hip/label_smooth.hip) and this module agree byte
for byte.

For every frame and every pixel ``p = (x, y)`` of the letterbox-valid crop ``L = labels[:crop_h,
:crop_w]``:

* ``W(p)`` is the set of crop pixels ``q`` with ``|qx - x| <= R`` and ``|qy - y| <= R``: the window
  is clipped to the crop; pixels outside it do not vote and are not replicated.
* ``v(c) = #{q in W(p) : L[q] == c}`` and ``m = max_c v(c)``.
* The output is ``L[p]`` if ``v(L[p]) == m`` (the centre keeps its label on a tie it takes part
  in), otherwise the smallest ``c`` with ``v(c) == m``.
* Any uint8 value is a label, 255 included; nothing depends on the number of classes.
* With a confidence plane ``K``, a pixel whose label did not change keeps ``K[p]``; a changed
  pixel gets ``floor(sum{K[q] : q in W(p), L[q] == out} / v(out))`` (the sum is at most 49 * 255).
* Pixels of the ``H x W`` plane outside the crop pass through, labels and codes alike.
* All votes read the raw input plane: one pass, no iteration.

``apply`` is the implementation (box counts per label present, from 2-D cumulative sums);
``apply_slow`` is the definition spelled out pixel by pixel, which the tests hold ``apply`` to.
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np

MIN_RADIUS, MAX_RADIUS = 1, 3


def check_params(R: int) -> None:
    """Raise unless ``R`` is a valid window radius."""
    if not MIN_RADIUS <= int(R) <= MAX_RADIUS:
        raise ValueError(f"--smooth_labels {R} outside {MIN_RADIUS} .. {MAX_RADIUS} (0: off)")


def _planes(labels, conf, crop_w: int, crop_h: int, R: int):
    check_params(R)
    lab = np.asarray(labels)
    if lab.dtype != np.uint8 or lab.ndim != 3:
        raise ValueError(f"smooth: labels {lab.dtype} {lab.shape} are not uint8 [B, H, W]")
    if not (1 <= int(crop_h) <= lab.shape[1] and 1 <= int(crop_w) <= lab.shape[2]):
        raise ValueError(f"smooth: crop {crop_w} x {crop_h} outside the map {lab.shape[1:]}")
    cf = None
    if conf is not None:
        cf = np.asarray(conf)
        if cf.dtype != np.uint8 or cf.shape != lab.shape:
            raise ValueError(f"smooth: conf {cf.dtype} {cf.shape} != labels uint8 {lab.shape}")
    return lab, cf


def _box(plane: np.ndarray, y0, y1, x0, x1) -> np.ndarray:
    """Sums of int32 ``plane`` [B, h, w] over the windows [y0, y1) x [x0, x1) of every pixel."""
    I = np.zeros((plane.shape[0], plane.shape[1] + 1, plane.shape[2] + 1), np.int32)
    np.cumsum(np.cumsum(plane, axis=1, dtype=np.int32), axis=2, out=I[:, 1:, 1:])
    return I[:, y1, x1] - I[:, y0, x1] - I[:, y1, x0] + I[:, y0, x0]


def apply(labels, conf, crop_w: int, crop_h: int, R: int) -> Tuple[np.ndarray, Optional[np.ndarray]]:
    """``labels`` uint8 [B, H, W], ``conf`` their confidence codes or None -> (smoothed labels,
    smoothed codes or None), new arrays of the same shapes; the inputs are not written."""
    lab, cf = _planes(labels, conf, crop_w, crop_h, R)
    crop_w, crop_h, R = int(crop_w), int(crop_h), int(R)
    out = lab.copy()
    cout = None if cf is None else cf.copy()
    L = lab[:, :crop_h, :crop_w]
    ys, xs = np.arange(crop_h)[:, None], np.arange(crop_w)[None, :]
    win = (np.maximum(ys - R, 0), np.minimum(ys + R + 1, crop_h),
           np.maximum(xs - R, 0), np.minimum(xs + R + 1, crop_w))
    K = None if cf is None else cf[:, :crop_h, :crop_w].astype(np.int32)
    best_v = np.zeros(L.shape, np.int32)      # the largest count so far, labels in ascending order
    best_c = np.zeros(L.shape, np.uint8)      # ... and the smallest label that has it
    own_v = np.zeros(L.shape, np.int32)       # the count of the pixel's own label
    best_k = None if K is None else np.zeros(L.shape, np.int32)
    for c in np.unique(L):
        is_c = L == c
        v = _box(is_c.astype(np.int32), *win)
        np.copyto(own_v, v, where=is_c)
        up = v > best_v
        np.copyto(best_v, v, where=up)
        best_c[up] = c
        if K is not None:
            np.copyto(best_k, _box(np.where(is_c, K, 0), *win), where=up)
    changed = own_v != best_v
    res = np.where(changed, best_c, L)
    out[:, :crop_h, :crop_w] = res
    if K is not None:
        mean = best_k // np.maximum(best_v, 1)
        cout[:, :crop_h, :crop_w] = np.where(changed, mean, K).astype(np.uint8)
    return out, cout


def apply_slow(labels, conf, crop_w: int, crop_h: int, R: int) -> Tuple[np.ndarray, Optional[np.ndarray]]:
    """The definition pixel by pixel, deliberately naive: what ``apply`` must equal."""
    lab, cf = _planes(labels, conf, crop_w, crop_h, R)
    crop_w, crop_h, R = int(crop_w), int(crop_h), int(R)
    out = lab.copy()
    cout = None if cf is None else cf.copy()
    for b in range(lab.shape[0]):
        L = lab[b, :crop_h, :crop_w].tolist()
        K = None if cf is None else cf[b, :crop_h, :crop_w].tolist()
        for y in range(crop_h):
            for x in range(crop_w):
                votes, codes = {}, {}
                for qy in range(max(0, y - R), min(crop_h, y + R + 1)):
                    for qx in range(max(0, x - R), min(crop_w, x + R + 1)):
                        c = L[qy][qx]
                        votes[c] = votes.get(c, 0) + 1
                        if K is not None:
                            codes[c] = codes.get(c, 0) + K[qy][qx]
                m = max(votes.values())
                own = L[y][x]
                if votes[own] == m:
                    continue
                win = min(c for c, v in votes.items() if v == m)
                out[b, y, x] = win
                if K is not None:
                    cout[b, y, x] = codes[win] // votes[win]
    return out, cout
