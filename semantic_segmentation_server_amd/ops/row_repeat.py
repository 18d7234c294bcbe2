"""The letterbox's constant rows, computed once: the host mirror of csrc/hip/row_repeat.h.

The letterbox pads bottom / right, so model-input rows ``[p0, H)`` are the constant -1 across
the full width. The front layers are 3x3 pad-1 conv chains that run the same arithmetic
for every row: an output row whose whole vertical receptive field lies in ``[p0, H - 1]``
equals the row above it bit for bit. ``stem_band`` and ``fused_ir_slice`` derive that run
of rows on the device from the LUT in use and compute it once; the plan builder passes
them the layer's cumulative receptive field from here.

A receptive field is ``(s, a, b)``: output row ``o`` reads model-input rows
``[s * o - a, s * o + b]``. The model input itself is ``(1, 0, 0)``.
"""
from __future__ import annotations

import os
from typing import Optional, Sequence, Tuple

RF = Tuple[int, int, int]
RF_INPUT: RF = (1, 0, 0)


def mode() -> str:
    """``SSA_ROW_REPEAT``, read at plan build: ``0`` = off (A/B runs, tests); ``all`` = on in
    every kernel that has it, whether it pays or not (tests); anything else = on where the
    plan builder expects it to pay (the default)."""
    v = os.environ.get("SSA_ROW_REPEAT", "1")
    return "off" if v == "0" else "all" if v == "all" else "auto"


def enabled() -> bool:
    return mode() != "off"


def rf_conv3x3(rf: RF, stride: int = 1, dilation: int = 1) -> RF:
    """The receptive field after a 3x3 pad-``dilation`` conv on top of ``rf``. (A 1x1 conv
    leaves it unchanged.)"""
    s, a, b = rf
    return (s * stride, s * dilation + a, s * dilation + b)


def pad_start(lut_y: Sequence[int]) -> int:
    """Start of the trailing run of pad rows: ``1 + max{y : lut_y[y] != -1}``, 0 if none."""
    p0 = 0
    for y, v in enumerate(lut_y):
        if int(v) != -1:
            p0 = y + 1
    return p0


def zone(p0: int, H: int, OH: int, rf: RF) -> Optional[Tuple[int, int]]:
    """Output rows ``[z0, z1)`` that equal row ``z0``: ``s o - a >= p0`` and ``s o + b <=
    H - 1`` (rows at or past ``H`` are zero padding, not -1). None: fewer than 2 rows."""
    s, a, b = rf
    if s < 1 or H - 1 - b < 0:
        return None
    z0 = -(-(p0 + a) // s)
    z1 = min(OH, (H - 1 - b) // s + 1)
    return (z0, z1) if z1 - z0 >= 2 else None


def band_segments(zn: Optional[Tuple[int, int]], OH: int, R: int, by: int):
    """Real output rows of band ``by`` of ``ceil(OH / R)``: the bands are laid out over the
    rows that still need computing, ``[0, z0] u [z1, OH)``; mapped back that is at most two
    ``(y0, y1)`` segments."""
    nby = -(-OH // R)
    if zn is None:
        y0 = by * R
        return [(y0, min(y0 + R, OH))] if y0 < OH else []
    z0, z1 = zn
    nrep = z1 - z0 - 1
    nc = OH - nrep
    rp = -(-nc // nby)
    c0, c1 = by * rp, min((by + 1) * rp, nc)
    segs = [(c0, min(c1, z0 + 1)), (max(c0, z0 + 1) + nrep, c1 + nrep)]
    return [(y0, y1) for y0, y1 in segs if y0 < y1]


def pays(p0: int, H: int, OH: int, R: int, rf: RF) -> bool:
    """Does a launch with bands of ``R`` rows get shorter bands from the zone? The grid stays
    ``ceil(OH / R)`` bands, so the gain is ``R' < R`` with ``R' = ceil(Nc / nby)``; where no
    band gets shorter the kernel would only pay for finding the zone."""
    zn = zone(p0, H, OH, rf)
    if zn is None:
        return False
    nby = -(-OH // R)
    return -(-(OH - (zn[1] - zn[0] - 1)) // nby) < R
