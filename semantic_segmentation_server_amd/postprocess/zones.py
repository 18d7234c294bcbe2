"""Zone occupancy: per frame, the pixel count of every class inside every zone of the picture
(``--serve_zones``, v2 GetZoneOccupancy). This file is the one definition: the oracle of the
device kernel (csrc/hip/zone_stats.hip), the implementation of the CPU / ``--backend torch`` /
host post-processing paths, and the decoder behind the RPC.

**Zone file** (``--zones FILE.json``)::

    {"zones": [{"name": "door", "polygon": [[x, y], ...]},
               {"name": "bay", "rect": [x0, y0, x1, y1]}, ...]}

Coordinates are fractions of the camera frame (0..1, origin top-left); values outside 0..1 are
allowed (up to ``MAX_COORD`` in magnitude) and simply fall outside the crop. 0..32 zones, names
unique, non-empty and not ``"frame"``; a polygon has at least 3 vertices; zones may overlap.

**Rasterisation** (``rasterize``), once per camera geometry, in exact integers. The letterbox
puts the camera frame into ``labels[:crop_h, :crop_w]``, so a vertex maps to the sub-pixel
integers ``X = floor(x * crop_w * 256 + 0.5)``, ``Y = floor(y * crop_h * 256 + 0.5)``. Pixel
``(px, py)`` is in the zone iff its centre ``(256 px + 128, 256 py + 128)`` is inside the polygon
by the even-odd rule, decided edge by edge: horizontal edges are skipped; every other edge is
oriented so that ``Y0 < Y1`` and counts iff ``Y0 <= cy < Y1`` and ``(cx - X0) * (Y1 - Y0) <
(X1 - X0) * (cy - Y0)`` in int64. Half-open in y and strict in x: two zones that share an edge
never both own a pixel and never both miss it, and the order and the starting vertex of a
polygon do not matter. The result is ``plane = uint32[crop_h, crop_w]`` with bit ``z - 1`` set
iff the pixel is in user zone ``z = 1 .. Z``. Zone 0 is implicit: the whole crop, named
``"frame"``; it is not in the plane.

**Statistics** (``encode``): ``R = 1 + Z`` rows, ``C`` classes, ``N = crop_h * crop_w``::

    pixels[r][c]   = #{ i : labels[i] == c and (r == 0 or bit r - 1 of plane[i]) }
    sum_conf[r][c] = the sum of conf[i] over the same pixels     (with a confidence plane)

Pixels whose label is ``>= C`` count nowhere. A frame's words are ``uint32[4 + R C]``, or
``uint32[4 + 2 R C]`` with confidence: the header ``R, N, crop_w, crop_h``, the ``pixels`` block
row-major ``[r][c]``, then the ``sum_conf`` block in the same order. Every word is written every
time, zeros included.

**Limits** (``check_geometry``): ``N < 2^24`` (so ``sum_conf <= 255 N < 2^32``), ``Z <= 32``,
``C <= 256``, ``R C <= ZONE_COUNTERS`` (the kernel's on-chip table).
"""
from __future__ import annotations

import json
import logging
import math
from typing import List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

log = logging.getLogger(__name__)

MAX_ZONES = 32
MAX_CLASSES = 256
ZONE_COUNTERS = 4096       # R * C counters of one frame (the kernel's LDS table)
MAX_PIXELS = 1 << 24       # N < 2^24: 255 * N fits a word
MAX_COORD = 1024.0         # largest magnitude of a normalised coordinate
FRAME = "frame"            # the name of the implicit zone 0
SUB = 256                  # sub-pixel units per pixel


class Zone(NamedTuple):
    name: str
    polygon: Tuple[Tuple[float, float], ...]  # normalised (x, y) vertices, at least 3


def _num(v, where: str) -> float:
    if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(float(v)):
        raise ValueError(f"{where}: coordinate {v!r} is not a finite number")
    if abs(float(v)) > MAX_COORD:
        raise ValueError(f"{where}: coordinate {v!r} is outside +-{MAX_COORD:g}")
    return float(v)


def parse(obj, source: str = "<zones>") -> List[Zone]:
    """The zones of a decoded zone file; ``source`` names the file in the errors."""
    if not isinstance(obj, dict) or not isinstance(obj.get("zones"), list):
        raise ValueError(f'{source}: expected an object {{"zones": [...]}}')
    raw = obj["zones"]
    if len(raw) > MAX_ZONES:
        raise ValueError(f"{source}: {len(raw)} zones, at most {MAX_ZONES} are served "
                         f"(the first one over is zone {MAX_ZONES + 1}, "
                         f"{raw[MAX_ZONES].get('name') if isinstance(raw[MAX_ZONES], dict) else None!r})")
    zones: List[Zone] = []
    seen = set()
    for k, z in enumerate(raw):
        if not isinstance(z, dict):
            raise ValueError(f"{source}: zone {k + 1} is not an object")
        name = z.get("name")
        where = f"{source}: zone {k + 1} ({name!r})"
        if not isinstance(name, str) or not name:
            raise ValueError(f"{where}: the name must be a non-empty string")
        if name == FRAME:
            raise ValueError(f'{where}: the name "{FRAME}" is the implicit whole-frame zone 0')
        if name in seen:
            raise ValueError(f"{where}: the name is used twice")
        seen.add(name)
        if ("polygon" in z) == ("rect" in z):
            raise ValueError(f'{where}: exactly one of "polygon" and "rect" is required')
        if "rect" in z:
            r = z["rect"]
            if not isinstance(r, (list, tuple)) or len(r) != 4:
                raise ValueError(f'{where}: "rect" must be [x0, y0, x1, y1]')
            x0, y0, x1, y1 = (_num(v, where) for v in r)
            poly = ((x0, y0), (x1, y0), (x1, y1), (x0, y1))
        else:
            p = z["polygon"]
            if not isinstance(p, (list, tuple)) or len(p) < 3:
                n = len(p) if isinstance(p, (list, tuple)) else 0
                raise ValueError(f"{where}: a polygon needs at least 3 vertices, got {n}")
            for v in p:
                if not isinstance(v, (list, tuple)) or len(v) != 2:
                    raise ValueError(f"{where}: vertex {v!r} is not [x, y]")
            poly = tuple((_num(v[0], where), _num(v[1], where)) for v in p)
        zones.append(Zone(name, poly))
    return zones


def load(path: str) -> List[Zone]:
    """The zones of ``--zones FILE.json``; errors name the file and the zone."""
    try:
        with open(path) as f:
            obj = json.load(f)
    except (OSError, ValueError) as e:
        raise ValueError(f"--zones {path}: cannot read the zone file ({e})") from e
    return parse(obj, f"--zones {path}")


def names(zones: Sequence[Zone]) -> List[str]:
    """The names of the R = 1 + Z rows: ``"frame"``, then the user zones."""
    return [FRAME] + [z.name for z in zones]


def vertices(zone: Zone, crop_w: int, crop_h: int) -> np.ndarray:
    """int64 [V, 2] sub-pixel (X, Y) of the zone's vertices in a ``crop_w x crop_h`` crop."""
    return np.array([[math.floor(x * crop_w * SUB + 0.5), math.floor(y * crop_h * SUB + 0.5)]
                     for x, y in zone.polygon], np.int64)


def inside(v: np.ndarray, crop_w: int, crop_h: int) -> np.ndarray:
    """bool [crop_h, crop_w]: the pixels whose centre is inside the polygon of the sub-pixel
    vertices ``v`` (int64 [V, 2]) by the edge rule of this file."""
    v = np.asarray(v, np.int64)
    lim = 1 << 30  # differences < 2^31, products < 2^62
    if SUB * max(crop_w, crop_h) >= lim or (len(v) and int(np.abs(v).max()) >= lim):
        raise ValueError("zones: vertex or crop too large for the exact int64 edge test")
    cx = (SUB * np.arange(crop_w, dtype=np.int64) + SUB // 2)[None, :]
    cy = SUB * np.arange(crop_h, dtype=np.int64) + SUB // 2
    out = np.zeros((crop_h, crop_w), bool)
    for k in range(len(v)):
        (x0, y0), (x1, y1) = v[k], v[(k + 1) % len(v)]
        if y0 == y1:
            continue
        if y0 > y1:
            x0, y0, x1, y1 = x1, y1, x0, y0
        rows = np.nonzero((cy >= y0) & (cy < y1))[0]
        if len(rows) == 0:
            continue
        lo, hi = int(rows[0]), int(rows[-1]) + 1  # the rows of an edge are consecutive
        out[lo:hi] ^= (cx - x0) * (y1 - y0) < (x1 - x0) * (cy[lo:hi, None] - y0)
    return out


def rasterize(zones: Sequence[Zone], crop_w: int, crop_h: int, warn: bool = True) -> np.ndarray:
    """uint32 [crop_h, crop_w], contiguous: bit ``z - 1`` set iff the pixel is in user zone
    ``z``. A zone without a pixel is legal (it serves zeros); it is logged once here."""
    if len(zones) > MAX_ZONES:
        raise ValueError(f"zones: {len(zones)} zones, at most {MAX_ZONES}")
    plane = np.zeros((crop_h, crop_w), np.uint32)
    for k, z in enumerate(zones):
        m = inside(vertices(z, crop_w, crop_h), crop_w, crop_h)
        if warn and not m.any():
            log.warning("zone %d (%r) covers no pixel of the %d x %d crop: it serves zeros",
                        k + 1, z.name, crop_w, crop_h)
        plane |= m.astype(np.uint32) << np.uint32(k)
    return np.ascontiguousarray(plane)


def check_geometry(crop_w: int, crop_h: int, num_zones: int, num_classes: int) -> None:
    """Raise unless ``--serve_zones`` can serve ``num_zones`` user zones of ``num_classes``
    classes in a ``crop_w x crop_h`` crop."""
    if crop_w < 1 or crop_h < 1:
        raise ValueError(f"--serve_zones: empty crop {crop_w} x {crop_h}")
    if crop_w * crop_h >= MAX_PIXELS:
        raise ValueError(f"--serve_zones: {crop_w} x {crop_h} = {crop_w * crop_h} pixels; a zone's "
                         f"confidence sum needs fewer than 2^24 = {MAX_PIXELS}")
    if not 0 <= num_zones <= MAX_ZONES:
        raise ValueError(f"--serve_zones: {num_zones} zones, at most {MAX_ZONES} (--zones)")
    if not 1 <= num_classes <= MAX_CLASSES:
        raise ValueError(f"--serve_zones: {num_classes} classes, 1 .. {MAX_CLASSES} (--num_classes)")
    if (1 + num_zones) * num_classes > ZONE_COUNTERS:
        raise ValueError(f"--serve_zones: (1 + {num_zones} zones) x {num_classes} classes = "
                         f"{(1 + num_zones) * num_classes} counters, at most {ZONE_COUNTERS}: "
                         f"{num_classes} classes allow {ZONE_COUNTERS // num_classes - 1} zones (--zones)")


def frame_words(rows: int, num_classes: int, conf: bool = False) -> int:
    """Words of one frame: the header and one (two with confidence) [R][C] blocks."""
    return 4 + rows * num_classes * (2 if conf else 1)


def rows_of(plane: Optional[np.ndarray]) -> int:
    """The fewest rows that hold every bit set in ``plane`` (1 without a plane)."""
    if plane is None or plane.size == 0:
        return 1
    return 1 + int(np.bitwise_or.reduce(np.asarray(plane, np.uint32), axis=None)).bit_length()


def encode(labels: np.ndarray, plane: Optional[np.ndarray], crop_w: int, crop_h: int, C: int,
           conf: Optional[np.ndarray] = None, out: Optional[np.ndarray] = None,
           rows: Optional[int] = None) -> np.ndarray:
    """The frame words of one label map ``labels`` (uint8 [H, W], read inside the crop) against
    ``plane`` (uint32 [crop_h, crop_w], or None: the frame row alone). ``rows``: R = 1 + Z (default:
    the fewest rows that hold the plane's bits); ``conf``: the uint8 [H, W] confidence plane of
    ``labels``; ``out``: where the words go (all of them are written)."""
    R = rows_of(plane) if rows is None else int(rows)
    C = int(C)
    if plane is None and R != 1:
        raise ValueError(f"zones.encode: {R} rows need a zone plane")
    check_geometry(crop_w, crop_h, R - 1, C)
    N = crop_w * crop_h
    lab = np.asarray(labels)[:crop_h, :crop_w].reshape(-1).astype(np.int64)
    if lab.size != N:
        raise ValueError(f"zones.encode: labels {np.asarray(labels).shape} do not hold the "
                         f"{crop_w} x {crop_h} crop")
    cf = None
    if conf is not None:
        cf = np.asarray(conf)[:crop_h, :crop_w].reshape(-1).astype(np.float64)  # sums < 2^32: exact
    pl = None
    if plane is not None:
        pl = np.asarray(plane)
        if pl.shape != (crop_h, crop_w):
            raise ValueError(f"zones.encode: plane {pl.shape} != ({crop_h}, {crop_w})")
        pl = pl.reshape(-1).astype(np.uint32)
    nw = frame_words(R, C, cf is not None)
    if out is None:
        out = np.zeros(nw, np.uint32)
    elif out.shape != (nw,) or out.dtype != np.uint32:
        raise ValueError(f"zones.encode: out must be uint32[{nw}]")
    out[:4] = (R, N, crop_w, crop_h)
    valid = lab < C
    for r in range(R):
        sel = valid if r == 0 else valid & ((pl >> np.uint32(r - 1)) & np.uint32(1)).astype(bool)
        ls = lab[sel]
        out[4 + r * C:4 + (r + 1) * C] = np.bincount(ls, minlength=C).astype(np.uint32)
        if cf is not None:
            o = 4 + (R + r) * C
            out[o:o + C] = np.bincount(ls, weights=cf[sel], minlength=C).astype(np.uint32)
    return out


class ZoneStats(NamedTuple):
    rows: int               # R = 1 + Z
    n: int                  # N = crop_w * crop_h
    crop_w: int
    crop_h: int
    pixels: np.ndarray      # uint32 [R, C]
    sum_conf: Optional[np.ndarray]  # uint32 [R, C], or None without confidence


def decode(words: np.ndarray, conf: bool = False) -> ZoneStats:
    """The header and the [R, C] blocks of one frame's words (views of ``words``)."""
    w = np.asarray(words)
    if w.dtype != np.uint32:
        w = w.view(np.uint32)
    if w.ndim != 1 or len(w) < 4:
        raise ValueError("zones.decode: expected one frame's uint32 words")
    R = int(w[0])
    blocks = 2 if conf else 1
    if R < 1 or (len(w) - 4) % (R * blocks) or len(w) == 4:
        raise ValueError(f"zones.decode: {len(w)} words do not hold {R} rows"
                         f"{' with confidence' if conf else ''}")
    C = (len(w) - 4) // (R * blocks)
    px = w[4:4 + R * C].reshape(R, C)
    sc = w[4 + R * C:4 + 2 * R * C].reshape(R, C) if conf else None
    return ZoneStats(R, int(w[1]), int(w[2]), int(w[3]), px, sc)
