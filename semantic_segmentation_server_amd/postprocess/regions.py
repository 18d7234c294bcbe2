"""Class regions of label maps: the numpy definition of the format.

A *region* is a maximal **8-connected** set of pixels of **one class** inside the
letterbox-valid crop ``labels[:crop_h, :crop_w]``, for the classes of a served set (a 256-bit
mask; by default every class id in ``1 .. num_classes - 1``). Pixels of classes outside the set
belong to no region and connect nothing. With the flat crop index ``i = y * crop_w + x``, a
region R has

    root                           the smallest i in R (its first pixel in raster order)
    pixels                         |R|
    sum_x, sum_y                   exact integer sums of the pixel coordinates
    x_min, y_min, x_max, y_max     the bounding box (inclusive)

A region *passes* if ``pixels >= min_pixels``; passing regions are ordered by ``pixels``
descending, then ``root`` ascending. Per frame, on the device and on the host,
``uint32[4 + 6 * K]``::

    word 0   n_regions, the true number of passing regions (may exceed K)
    word 1   N = crop_w * crop_h
    word 2   crop_w
    word 3   crop_h
    then six words for each of the first min(n_regions, K) regions in that order:
      0  (label << 24) | root      3  sum_y
      1  pixels                    4  x_min | (y_min << 16)
      2  sum_x                     5  x_max | (y_max << 16)

Words past the used ones are not written.

With a per-pixel confidence plane (uint8 codes beside the labels, ``--serve_confidence``) a
region has a seventh word, ``6  sum_conf``: the exact integer sum of the codes of its pixels
(``pixels < 2^24`` and codes ``<= 255``, so it fits 32 bits), and a frame is
``uint32[4 + 7 * K]`` with the same header. The mean confidence of a region is
``sum_conf / (255 * pixels)``.

With region tracks (``--track_regions``, postprocess/tracks.py) two more words follow the others
of a record, ``track_id`` and ``age`` (at 6 and 7, or at 7 and 8 with ``sum_conf``), and a frame
is ``uint32[4 + (6 | 7 + 2) * K]`` with the same header.

This module is the oracle of the device kernels (``csrc/hip/class_regions.hip``), the encoder
of the CPU / torch / exact paths, and the decoder of the RPC.
"""
from __future__ import annotations

from typing import Iterable, Optional, Union

import numpy as np

HEADER = 4
WORDS = 6                      # per region
WORDS_CONF = 7                 # per region with sum_conf
WORDS_TRACK = 2                # more per region with track_id, age
MAX_PIXELS = 1 << 24           # a root is stored in 24 bits
MAX_REGIONS = 256              # K
REGION_CANDIDATES = 4096       # most regions that may pass in a frame (the kernel file's constant)

REGION_DTYPE = np.dtype([("label", np.uint8), ("root", np.uint32), ("pixels", np.uint32),
                         ("sum_x", np.uint32), ("sum_y", np.uint32),
                         ("x_min", np.uint16), ("y_min", np.uint16),
                         ("x_max", np.uint16), ("y_max", np.uint16), ("sum_conf", np.uint32),
                         ("track_id", np.uint32), ("age", np.uint32)])


def words_per_region(conf: bool = False, tracks: bool = False) -> int:
    return (WORDS_CONF if conf else WORDS) + (WORDS_TRACK if tracks else 0)

Classes = Union[int, Iterable[int]]


def class_mask(classes: Classes) -> int:
    """The 256-bit served set as a Python int (bit c: class c). An int is taken as a mask."""
    if isinstance(classes, (int, np.integer)):
        m = int(classes)
        if m < 0 or m >> 256:
            raise ValueError("regions: the class set is a 256-bit mask")
        return m
    m = 0
    for c in classes:
        c = int(c)
        if not 0 <= c <= 255:
            raise ValueError(f"regions: class id {c} outside 0 .. 255")
        m |= 1 << c
    return m


def default_classes(num_classes: int) -> int:
    """Every class id in 1 .. num_classes - 1 (background excluded)."""
    return class_mask(range(1, max(1, min(256, int(num_classes)))))


def min_pixels_for(ratio: float, H: int, W: int) -> int:
    """``ceil(ratio * H * W)`` of the model input, at least 1."""
    return max(1, int(np.ceil(float(ratio) * H * W - 1e-9)))


def check_geometry(crop_w: int, crop_h: int, min_pixels: int, K: int) -> None:
    """Raise ValueError, naming the flag to change, unless the regions of a ``crop_h x crop_w``
    map are encodable with ``K`` records and a ``min_pixels`` threshold."""
    if crop_w < 1 or crop_h < 1:
        raise ValueError(f"regions: empty crop {crop_h} x {crop_w}")
    n = crop_w * crop_h
    if n >= MAX_PIXELS:
        raise ValueError(f"regions: {crop_h} x {crop_w} = {n} pixels do not fit a 24-bit root "
                         f"(N < {MAX_PIXELS} required; lower --input_size)")
    if n * max(crop_w, crop_h) >= 1 << 32:
        raise ValueError(f"regions: the coordinate sums of a {crop_h} x {crop_w} map do not fit "
                         "32 bits (N * max(crop_w, crop_h) < 2^32 required; lower --input_size)")
    if K < 1 or K > MAX_REGIONS:
        raise ValueError(f"regions: --max_regions {K} outside 1 .. {MAX_REGIONS}")
    if min_pixels < 1:
        raise ValueError(f"regions: min_pixels {min_pixels} < 1 (raise --region_min_area_ratio)")
    if n // min_pixels > REGION_CANDIDATES:
        raise ValueError(f"regions: up to {n // min_pixels} regions of {min_pixels} pixels fit a "
                         f"{crop_h} x {crop_w} map, more than the {REGION_CANDIDATES} candidates "
                         "the selection holds (raise --region_min_area_ratio)")


def label_components(labels: np.ndarray, mask: int) -> np.ndarray:
    """int64[h, w]: per pixel the smallest flat index of its region, -1 for pixels of classes
    outside ``mask``. Plain numpy: min-label hooking over the same-class 8-neighbour pairs,
    then pointer jumping, until every pair agrees."""
    h, w = labels.shape
    served = np.array([(mask >> c) & 1 for c in range(256)], bool)[labels]
    idx = np.arange(h * w, dtype=np.int64).reshape(h, w)
    us, vs = [], []
    for dy, dx in ((0, 1), (1, 0), (1, 1), (1, -1)):
        a = (slice(0, h - dy), slice(max(0, -dx), w - max(0, dx)))
        b = (slice(dy, h), slice(max(0, dx), w + min(0, dx)))
        same = served[a] & (labels[a] == labels[b])
        us.append(idx[a][same])
        vs.append(idx[b][same])
    u, v = np.concatenate(us), np.concatenate(vs)
    L = np.arange(h * w, dtype=np.int64)
    while True:
        a, b = L[u], L[v]
        diff = a != b
        if not diff.any():
            break
        u, v, a, b = u[diff], v[diff], a[diff], b[diff]
        np.minimum.at(L, np.maximum(a, b), np.minimum(a, b))
        while True:
            LL = L[L]
            if np.array_equal(LL, L):
                break
            L = LL
    L = L.reshape(h, w)
    L[~served] = -1
    return L


def region_table(labels: np.ndarray, crop_w: int, crop_h: int, classes: Classes,
                 min_pixels: int = 1, conf: Optional[np.ndarray] = None) -> np.ndarray:
    """REGION_DTYPE[n]: every passing region of the crop, in the output order. ``sum_conf``
    is summed from ``conf`` (a uint8 map beside ``labels``) and 0 without it; ``track_id`` and
    ``age`` are 0 (postprocess/tracks.py fills them)."""
    return table_and_roots(labels, crop_w, crop_h, classes, min_pixels, conf)[0]


def table_and_roots(labels: np.ndarray, crop_w: int, crop_h: int, classes: Classes,
                    min_pixels: int = 1, conf: Optional[np.ndarray] = None):
    """(``region_table``, int64[crop_h * crop_w]: per pixel the root of its region, -1 outside
    the class set)."""
    lab = np.ascontiguousarray(np.asarray(labels)[:crop_h, :crop_w])
    roots = label_components(lab, class_mask(classes)).reshape(-1)
    on = np.flatnonzero(roots >= 0)
    out = np.zeros(0, REGION_DTYPE)
    if on.size == 0:
        return out, roots
    r = roots[on]
    order = np.argsort(r, kind="stable")
    on, r = on[order], r[order]
    first = np.flatnonzero(np.concatenate(([True], r[1:] != r[:-1])))
    x, y = on % crop_w, on // crop_w
    root = r[first]
    pixels = np.diff(np.concatenate((first, [len(r)])))
    keep = pixels >= min_pixels
    tab = np.zeros(len(first), REGION_DTYPE)
    tab["label"] = lab.reshape(-1)[root]
    tab["root"], tab["pixels"] = root, pixels
    tab["sum_x"], tab["sum_y"] = np.add.reduceat(x, first), np.add.reduceat(y, first)
    tab["x_min"], tab["y_min"] = np.minimum.reduceat(x, first), np.minimum.reduceat(y, first)
    tab["x_max"], tab["y_max"] = np.maximum.reduceat(x, first), np.maximum.reduceat(y, first)
    if conf is not None:
        c = np.ascontiguousarray(np.asarray(conf)[:crop_h, :crop_w]).reshape(-1).astype(np.int64)
        tab["sum_conf"] = np.add.reduceat(c[on], first)
    tab = tab[keep]
    return tab[np.lexsort((tab["root"], -tab["pixels"].astype(np.int64)))], roots


def pack(tab: np.ndarray, conf: bool = False, tracks: bool = False) -> np.ndarray:
    """REGION_DTYPE[n] -> uint32[n, 6] record words ([n, 7] with ``conf``; two more, track_id
    and age, with ``tracks``)."""
    w = np.zeros((len(tab), words_per_region(conf, tracks)), np.uint32)
    if conf:
        w[:, 6] = tab["sum_conf"]
    if tracks:
        w[:, -2], w[:, -1] = tab["track_id"], tab["age"]
    w[:, 0] = (tab["label"].astype(np.uint32) << 24) | tab["root"]
    w[:, 1], w[:, 2], w[:, 3] = tab["pixels"], tab["sum_x"], tab["sum_y"]
    w[:, 4] = tab["x_min"].astype(np.uint32) | (tab["y_min"].astype(np.uint32) << 16)
    w[:, 5] = tab["x_max"].astype(np.uint32) | (tab["y_max"].astype(np.uint32) << 16)
    return w


def encode(labels: np.ndarray, crop_w: int, crop_h: int, classes: Classes, min_pixels: int,
           K: int, out: Optional[np.ndarray] = None, conf: Optional[np.ndarray] = None,
           tracker=None) -> np.ndarray:
    """``labels[H, W]`` uint8 -> ``uint32[4 + 6 K]``; with ``conf[H, W]`` uint8, the
    7-word records: ``uint32[4 + 7 K]``. Unwritten words keep ``out``'s values (zero without
    ``out``). With ``tracker`` (a ``tracks.StreamTracker``: the state of this frame's stream,
    advanced by this call) the records end in ``track_id`` and ``age``."""
    labels = np.asarray(labels)
    if labels.ndim != 2 or labels.dtype != np.uint8:
        raise ValueError("regions.encode: labels must be a 2-D uint8 map")
    check_geometry(crop_w, crop_h, min_pixels, K)
    if crop_h > labels.shape[0] or crop_w > labels.shape[1]:
        raise ValueError(f"regions.encode: crop {crop_h} x {crop_w} outside the "
                         f"{labels.shape[0]} x {labels.shape[1]} map")
    rw = words_per_region(conf is not None, tracker is not None)
    if conf is not None:
        conf = np.asarray(conf)
        if conf.shape != labels.shape or conf.dtype != np.uint8:
            raise ValueError("regions.encode: conf must be a uint8 map of the labels' shape")
    if out is None:
        out = np.zeros(HEADER + rw * K, np.uint32)
    elif out.shape != (HEADER + rw * K,) or out.dtype != np.uint32:
        raise ValueError(f"regions.encode: out must be uint32[4 + {rw} K]")
    tab, roots = table_and_roots(labels, crop_w, crop_h, classes, min_pixels, conf)
    total, k = len(tab), min(len(tab), K)
    tab = tab[:k]
    if tracker is not None:
        from . import tracks
        tab["track_id"], tab["age"] = tracker.update(tab, tracks.plane_of(roots, tab))
    out[0], out[1], out[2], out[3] = total, crop_w * crop_h, crop_w, crop_h
    out[HEADER:HEADER + rw * k] = pack(tab, conf is not None, tracker is not None).reshape(-1)
    return out


def used_words(words: np.ndarray, K: Optional[int] = None, conf: bool = False,
               tracks: bool = False) -> int:
    """Header + stored records: ``4 + 6 * min(n_regions, K)`` (``K`` defaults to the array's);
    7-word records with ``conf``, two more words with ``tracks``."""
    rw = words_per_region(conf, tracks)
    K = (len(words) - HEADER) // rw if K is None else K
    return HEADER + rw * min(int(words[0]), K)


def decode(words: np.ndarray, conf: bool = False, tracks: bool = False) -> np.ndarray:
    """``uint32[>= 4 + 6 * stored]`` -> REGION_DTYPE[stored], the stored regions in order
    (``stored = min(n_regions, slots of the array)``; ``words[0]`` is the true total). With
    ``conf`` the records have 7 words; without, ``sum_conf`` is 0. With ``tracks`` two more
    words, ``track_id`` and ``age``; without, both are 0."""
    WORDS = words_per_region(conf, tracks)
    words = np.asarray(words)
    if words.ndim != 1 or len(words) < HEADER:
        raise ValueError("regions: words must be a 1-D array with the 4 header words")
    words = words.view(np.uint32) if words.dtype == np.int32 else words.astype(np.uint32, copy=False)
    total, n, cw, ch = (int(v) for v in words[:HEADER])
    if n != cw * ch or n < 1 or n >= MAX_PIXELS or total > n:
        raise ValueError(f"regions: bad header (regions {total}, N {n}, crop {ch} x {cw})")
    stored = min(total, (len(words) - HEADER) // WORDS)
    w = words[HEADER:HEADER + WORDS * stored].reshape(stored, WORDS)
    tab = np.zeros(stored, REGION_DTYPE)
    tab["label"], tab["root"] = w[:, 0] >> np.uint32(24), w[:, 0] & np.uint32(0xFFFFFF)
    tab["pixels"], tab["sum_x"], tab["sum_y"] = w[:, 1], w[:, 2], w[:, 3]
    tab["x_min"], tab["y_min"] = w[:, 4] & np.uint32(0xFFFF), w[:, 4] >> np.uint32(16)
    tab["x_max"], tab["y_max"] = w[:, 5] & np.uint32(0xFFFF), w[:, 5] >> np.uint32(16)
    if conf:
        tab["sum_conf"] = w[:, 6]
    if tracks:
        tab["track_id"], tab["age"] = w[:, WORDS - 2], w[:, WORDS - 1]
    return tab
