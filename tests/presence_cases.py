"""Shared cases of the zone-presence tests (tests/test_presence_cpu.py, tests/test_presence_gpu.py):
the zones, the two streams of drifting rectangles, and their oracle rows by the numpy definition
(postprocess/presence.py on top of regions.py and tracks.py). No GPU is touched here.
"""
import functools

import numpy as np

from semantic_segmentation_server_amd.postprocess import presence as PR
from semantic_segmentation_server_amd.postprocess import regions as RG
from semantic_segmentation_server_amd.postprocess import tracks as TK
from semantic_segmentation_server_amd.postprocess import zones as ZN

SENT = 0x5A5A5A5A

# two zones that share the edge x = 0.5, and a triangle
ZONES = {"zones": [{"name": "left", "rect": [0.0, 0.0, 0.5, 1.0]},
                   {"name": "right", "rect": [0.5, 0.0, 1.0, 1.0]},
                   {"name": "tri", "polygon": [[0.1, 0.1], [0.9, 0.25], [0.4, 0.95]]}]}

# the sequences: a 33 x 45 map, a 30 x 40 crop (pitch != width), pixels outside the crop hold a
# served class
SH, SW, SCH, SCW = 33, 45, 30, 40
SCLS = [1, 2, 3, 4]
SK, SMP = 6, 3
TRACK_Q = 256      # tracks.quantize(0.25)
PRESENCE_Q = 512   # presence.quantize(0.5)


def zone_plane(cw, ch):
    return ZN.rasterize(ZN.parse(ZONES), cw, ch, warn=False)


def _blank():
    m = np.zeros((SH, SW), np.uint8)
    m[SCH:, :] = 4
    m[:, SCW:] = 4
    return m


@functools.lru_cache(maxsize=None)
def sequences():
    """(maps of stream 0 [8], maps of stream 1 [4]). Stream 0: a 10 x 10 block of class 1 drifts
    right across the shared edge x = 20 of the crop (three frames inside "left", the frame with
    exactly half of it on each side, the same with one pixel moved across, back, then it splits in
    two pieces); a block of class 2 sits still in the triangle. Stream 1: a block of class 2 drifts
    down through the triangle and a block of class 3 straddles the edge."""
    s0 = []
    for t, x0 in enumerate([5, 7, 9, 12, 15, 15, 15, 17]):
        m = _blank()
        m[10:20, x0:x0 + 10] = 1
        if t == 5:  # 49 pixels left of the edge, 51 right of it: still one region of 100
            m[10, 15] = 0
            m[10, 25] = 1
        if t == 7:  # a gap row: pieces of 60 and 30 pixels
            m[16, :] = 0
        m[22:27, 14:20] = 2
        s0.append(m)
    s1 = []
    for t in range(4):
        m = _blank()
        m[2 + 4 * t:10 + 4 * t, 12:18] = 2
        m[24:29, 17 + t:23 + t] = 3
        s1.append(m)
    return s0, s1


def oracle(seq, tracks=True, K=SK, min_pixels=SMP, classes=SCLS, geom=(SCH, SCW), plane=None,
           rows=4, q=PRESENCE_Q, track_q=TRACK_Q, conf=None):
    """Per frame of one stream's maps: (region row as served, presence row), sentinel-prefilled
    region rows as the device tests' buffers are."""
    ch, cw = geom
    plane = zone_plane(cw, ch) if plane is None and rows > 1 else plane
    tr = TK.StreamTracker(track_q) if tracks else None
    dw = PR.StreamDwell() if tracks else None
    out = []
    for k, m in enumerate(seq):
        rw = RG.words_per_region(conf is not None, tracks)
        reg = RG.encode(m, cw, ch, classes, min_pixels, K, out=np.full(4 + rw * K, SENT, np.uint32),
                        conf=None if conf is None else conf[k], tracker=tr)
        tab = RG.decode(reg, conf=conf is not None, tracks=True) if tracks else None
        out.append((reg, PR.encode(m, plane, cw, ch, classes, min_pixels, K, rows, q, tab=tab, dwell=dw)))
    return out


@functools.lru_cache(maxsize=None)
def sequence_oracles():
    s0, s1 = sequences()
    return oracle(s0), oracle(s1)
