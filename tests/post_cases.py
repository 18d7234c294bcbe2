"""Adversarial inputs of the contour-statistics pipeline (csrc/hip/postprocess.hip) at small
shapes: the case table and the helpers shared by tests/test_post_cases_cpu.py (the spec
against the exact tracer, and every case's path condition) and
tests/test_postprocess_topology_gpu.py (the device against the spec).

Most cases use a two-colour palette: class 0 black, class 1 white, threshold 127. The mask
stage (3x3 box blur of the palette colours, rounded, gray, > 127) is then a 3x3 majority
filter of the label map under REFLECT_101. A pixel checkerboard of the two classes maps to
itself (REFLECT_101 keeps parity), its foreground is one 8-component, and every background
pixel is a 4-component of its own: 513 tile-local roots in a full 32x32 tile.

Every case names the device path it is there for; ``check_path`` asserts, from the reference
(``palette_mask_numpy`` / ``label_components`` / ``component_segments``) alone, the condition
that puts it there.
"""
from collections import Counter
from dataclasses import dataclass
from typing import Callable, Tuple

import numpy as np

from semantic_segmentation_server_amd.labels import cityscapes_colormap, pascal_colormap
from semantic_segmentation_server_amd.postprocess import components as C
from semantic_segmentation_server_amd.postprocess.reference import palette_mask_numpy
from semantic_segmentation_server_amd.postprocess.synthetic import random_label_map

# Constants of csrc/hip/postprocess.hip that the path conditions use (copied: a case must not
# drift off its path unnoticed when one of them changes there, so change both together).
TILE = 32          # TW = TH: the local CCL tile
kTileCap = 64      # roots per tile with a rootpix slot; the rest go to the rovf list
kMergeCap = 12288  # tile-local roots per frame that the LDS merge handles; more: union-find fallback
kSortCap = 2048    # passing contours that assign_frame sorts; more: raster scan
kTSlots = 64       # components per block of the tile accumulation tables
kHash = 128        # components per block of the strip accumulation table
kMaxDepth = 16     # ancestor chain entries per record slot in finalize_frame
kAnc = 8           # ancestors cached per slot of the tile accumulation tables
kPoolPerFrame = 8192
kDenseBins = 32    # classes of the tile tables; more classes take the strip kernel
K_MAX = 256        # record slots: finalize_frame's LDS arrays

TWO_TONE = np.zeros((256, 3), np.int32)
TWO_TONE[1] = 255
TWO_TONE.setflags(write=False)


# ------------------------------------------------------------------ reference-side helpers
def tile_roots(mask: np.ndarray) -> Tuple[int, int]:
    """(total, per-tile maximum) of the tile-local roots of a reference mask: per 32x32 tile,
    its 8-connected foreground components plus its 4-connected background components, each
    labelled inside the tile alone.

    This is a Python copy (scipy) of what ``k_ccl_local`` of csrc/hip/postprocess.hip counts
    into ``ntroot[tile]`` and ``flag[4]``, not a report from the kernel of what it counted. It
    keeps a case on the path it is listed for (rovf list, compact merge, union-find fallback)
    when a shape is edited; what a case pins about the kernels are its records."""
    from scipy import ndimage as ndi
    fg = np.asarray(mask) > 0
    h, w = fg.shape
    s8 = np.ones((3, 3), bool)
    s4 = np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]], bool)
    total = most = 0
    for y0 in range(0, h, TILE):
        for x0 in range(0, w, TILE):
            t = fg[y0:y0 + TILE, x0:x0 + TILE]
            n = ndi.label(t, structure=s8)[1] + ndi.label(~t, structure=s4)[1]
            total += n
            most = max(most, n)
    return total, most


def mask_of(labels, palette):
    return palette_mask_numpy(np.asarray(labels, np.uint8), palette) > 0


def nodes_of(labels, palette):
    """(node, fg) of the spec: node = raster index + 1 of the component's first pixel, 0 = outside."""
    return C.label_components(mask_of(labels, palette))


def max_nodes_per_tile(node: np.ndarray) -> int:
    h, w = node.shape
    best = 0
    for y0 in range(0, h, TILE):
        for x0 in range(0, w, TILE):
            u = np.unique(node[y0:y0 + TILE, x0:x0 + TILE])
            best = max(best, int((u != 0).sum()))
    return best


def max_nodes_per_run(node: np.ndarray, run: int = 256) -> int:
    """Most distinct components (outside excluded) in any ``run`` consecutive raster pixels."""
    flat = node.ravel().tolist()
    cnt = Counter()
    best = 0
    for i, n in enumerate(flat):
        if n:
            cnt[n] += 1
        if i >= run:
            o = flat[i - run]
            if o:
                cnt[o] -= 1
                if cnt[o] == 0:
                    del cnt[o]
        best = max(best, len(cnt))
    return best


def fill_histogram(labels, palette, n, bins):
    """Class counts of the fill of the OUTER contour of foreground component ``n`` that has no
    holes: its own pixels."""
    node, fg = nodes_of(labels, palette)
    return np.bincount(np.asarray(labels)[node == n], minlength=bins)


# ------------------------------------------------------------------ builders
# each returns (labels[h, w] uint8, palette, bins, min_area, K); labels < bins
def checkerboard(h, w, phase=1):
    yy, xx = np.mgrid[0:h, 0:w]
    return ((yy + xx + phase) & 1).astype(np.uint8)


def build_rovf(min_area, K):
    return checkerboard(70, 75), TWO_TONE, 2, min_area, K


FB_H, FB_W = 180, 177


def fallback_labels():
    lab = checkerboard(FB_H, FB_W)
    lab[50:100, 60:120] = 1                         # blob: joins the checkerboard's foreground
    lab[57:93, 68:112] = 0                          # its hole
    lab[62:78, 72:92] = checkerboard(16, 20, 0)     # foreground with holes of its own in the hole
    lab[82:88, 96:104] = 1                          # a solid island in the hole
    return lab


def build_fallback(min_area, K):
    return fallback_labels(), TWO_TONE, 2, min_area, K


def build_tables():
    h, w = 100, 180
    lab = np.zeros((h, w), np.uint8)
    lab[3:30, 8:172] = 1                            # large blob above the band
    lab[10:22, 40:90] = 0                           # with a hole
    lab[30:48, :] = checkerboard(18, w, 0)          # the band: through 6 tile columns, 2 tile rows
    lab[48:52, :] = 1
    lab[52:97, 5:175] = 1                           # large blob below
    lab[60:90, 100:160] = 0
    lab[70:80, 120:140] = 1
    return lab, TWO_TONE, 2, 0.0, K_MAX


CORNERS = ((32, 32), (64, 32), (32, 64))            # (y, x) of the tile corner, in a 100x100 crop
EDGE_POINTS = ((45, 32), (32, 45))                  # the same contacts across one tile edge, off the corner


def _pair(lab, cy, cx, anti, v):
    if anti:   # (cy, cx - 1) and (cy - 1, cx)
        lab[cy:cy + 3, cx - 3:cx] = v
        lab[cy - 3:cy, cx:cx + 3] = v
    else:      # (cy - 1, cx - 1) and (cy, cx)
        lab[cy - 3:cy, cx - 3:cx] = v
        lab[cy:cy + 3, cx:cx + 3] = v


def build_corner(kind, cy, cx):
    """Two 3x3 label squares that meet only diagonally at the point (cy, cx): a tile corner, or
    (``tileedge``) a point of one tile edge, where the vertical edges' own diagonal unions
    (kinds 2 and 3 of ``k_ccl_edges``) or the horizontal edge's (kind 0) carry the contact.
    Each becomes a plus of 5 mask pixels, and the two corner pixels nearest the other square
    survive the majority filter (4 of their own + 1 of the other's): the masks touch across
    the point and nowhere else. ``bg``: the same two squares as class 0 inside a class-1 block."""
    lab = np.zeros((100, 100), np.uint8)
    if kind == "bg":
        lab[cy - 14:cy + 14, cx - 14:cx + 14] = 1
        _pair(lab, cy, cx, bg_anti(cy, cx), 0)
    else:
        _pair(lab, cy, cx, kind == "anti", 1)
    return lab, TWO_TONE, 2, 0.0, 64


def bg_anti(cy, cx):
    return (cy, cx) in ((64, 32), (32, 45))  # these hold the anti-diagonal background pair


THIN = ((1, 37), (37, 1), (2, 2), (1, 1), (2, 40), (40, 2))
EDGE_CROPS = ((32, 32), (33, 32), (32, 33), (31, 65), (65, 31), (97, 131))
EDGE_P = (0.3, 0.5, 0.6)


def build_bernoulli(h, w, p, seed, K):
    rng = np.random.default_rng(seed)
    return (rng.random((h, w)) < p).astype(np.uint8), TWO_TONE, 2, 0.0, K


def _blob_map(seed):
    return random_label_map(np.random.default_rng(seed), 97, 131, n_blobs=6, noise=0.01)


CITY_FG = (4, 5, 6, 7, 9, 10)   # Cityscapes train ids whose colour is brighter than gray 127


def build_bins(which):
    lab = _blob_map(11)
    if which in (21, 32):
        return lab, np.asarray(pascal_colormap(), np.int32), which, 0.0, 64
    if which == 19:   # the engine's Cityscapes setting: 19 classes, six of them bright
        m = np.arange(256)
        m[19], m[20], m[7], m[15] = 2, 3, 9, 4
        lab = m[lab].astype(np.uint8)
        rng = np.random.default_rng(12)
        spots = rng.random(lab.shape) < 0.01
        lab[spots] = rng.choice(CITY_FG, size=int(spots.sum()))
        return lab, np.asarray(cityscapes_colormap(), np.int32), 19, 0.0, 64
    assert which == 40
    pal = np.asarray(pascal_colormap(), np.int32).copy()
    for c in range(21, 40):
        pal[c] = (c, 2 * c, 3 * c)          # dark
    pal[35] = (255, 255, 255)               # two bright classes above 32
    pal[38] = (200, 220, 210)
    m = np.arange(256)
    m[19], m[20], m[12], m[11] = 39, 33, 36, 22
    lab = m[lab].astype(np.uint8)
    right = np.zeros(lab.shape, bool)
    right[:, lab.shape[1] // 2:] = True
    lab[right & (lab == 7)] = 35            # the left half keeps 7 / 15
    lab[right & (lab == 15)] = 38
    lab[90:97, 0:9] = 39                    # the last bin, dark
    return lab, pal, 40, 0.0, 64


def build_tie():
    """A 10 x 20 block, class 15 left and class 7 right. Both survive the blur except next to
    class 0, so the mask is the 8 x 18 interior: 72 pixels of each class. The first maximum
    (class 7) wins in numpy's argmax and in the device's strict compare."""
    lab = np.zeros((40, 50), np.uint8)
    lab[12:22, 11:21] = 15
    lab[12:22, 21:31] = 7
    return lab, np.asarray(pascal_colormap(), np.int32), 21, 0.0, 64


def area_labels():
    lab = np.zeros((50, 60), np.uint8)
    lab[9:21, 30:47] = 1
    return lab


def area_of_rectangle():
    segs = C.component_segments(area_labels(), 0.0, TWO_TONE)
    assert len(segs) == 1 and not segs[0][6]
    return float(segs[0][2])


def build_area(bump):
    a = area_of_rectangle()
    return area_labels(), TWO_TONE, 2, float(np.nextafter(a, np.inf)) if bump else a, 64


# ------------------------------------------------------------------ the table
@dataclass(frozen=True)
class Case:
    name: str
    path: str                    # the device path the case is there for
    build: Callable
    fg: int = 1                  # a bright and a dark class of the case's palette
    bg: int = 0
    pad: Tuple[int, int] = (0, 0)   # frame = crop + pad, random labels outside the crop
    any_accum: bool = False      # the records do not depend on the accumulation pass


def _cases():
    out = [
        Case("rovf_compact-area4", "rovf list on the compact merge", lambda: build_rovf(4.0, 64)),
        Case("rovf_compact-area0-K64", "rovf list, more than K contours pass", lambda: build_rovf(0.0, 64)),
        Case("scan_select", "raster-scan selection above kSortCap", lambda: build_rovf(0.0, K_MAX)),
        Case("fallback_small-area4", "union-find fallback with nested holes", lambda: build_fallback(4.0, 64)),
        Case("fallback_small-area0-K256", "union-find fallback and raster-scan selection",
             lambda: build_fallback(0.0, K_MAX)),
        Case("tables_full", "full LDS tables of the accumulation kernels", build_tables),
    ]
    for kind in ("diag", "anti", "bg"):
        for cy, cx in CORNERS:
            out.append(Case(f"corner_{kind}-{cy}-{cx}", "contact across a tile corner only",
                            lambda kind=kind, cy=cy, cx=cx: build_corner(kind, cy, cx)))
        for cy, cx in EDGE_POINTS:
            out.append(Case(f"tileedge_{kind}-{cy}-{cx}", "diagonal contact across one tile edge only",
                            lambda kind=kind, cy=cy, cx=cx: build_corner(kind, cy, cx)))
    for i, (h, w) in enumerate(THIN):
        out.append(Case(f"thin-{h}x{w}", "crops 1 or 2 pixels wide or high",
                        lambda h=h, w=w, i=i: build_bernoulli(h, w, 0.6, 100 + i, 64),
                        pad=(2, 3), any_accum=True))
    for p in EDGE_P:
        for i, (h, w) in enumerate(EDGE_CROPS):
            out.append(Case(f"edges32-p{p}-{h}x{w}", "crop sizes around the 32-pixel tile, inside a larger frame",
                            lambda h=h, w=w, p=p, i=i: build_bernoulli(h, w, p, 200 + 10 * i + int(10 * p), K_MAX),
                            pad=(5, 7)))
    out += [
        Case("bins-21", "class bins = the engine's PASCAL count", lambda: build_bins(21), fg=15),
        Case("bins-32", "class bins = 32", lambda: build_bins(32), fg=15),
        Case("bins-19", "class bins = the engine's Cityscapes count", lambda: build_bins(19), fg=9),
        Case("bins-40", "more than 32 bins: the strip kernel whatever accum says", lambda: build_bins(40),
             fg=38),
        Case("tie", "two classes in equal counts: the first maximum", build_tie, fg=15),
        Case("area_edge-keep", "polygon area == min_area: kept", lambda: build_area(False)),
        Case("area_edge-drop", "polygon area just below min_area: dropped", lambda: build_area(True)),
    ]
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

_BUILT = {}


def built(case: Case):
    """The case's (labels, palette, bins, min_area, K), built once."""
    if case.name not in _BUILT:
        lab, pal, bins, min_area, K = case.build()
        lab = np.ascontiguousarray(lab, np.uint8)
        assert int(lab.max()) < bins and K <= K_MAX
        lab.setflags(write=False)
        _BUILT[case.name] = (lab, pal, bins, float(min_area), int(K))
    return _BUILT[case.name]


# ------------------------------------------------------------------ expectations (the spec)
_EXPECT = {}


def expected(key, labels, palette, min_area, K):
    """(records of the spec with K slots, more than K contours passed), cached by ``key``."""
    if key not in _EXPECT:
        more = C.component_segments(labels, min_area, palette, max_records=K + 1)
        over = len(more) > K
        exp = C.component_segments(labels, min_area, palette, max_records=K) if over else more
        _EXPECT[key] = (exp, over)
    return _EXPECT[key]


def plain_frame(h, w, fg, bg):
    """A blob with a hole and an island: a handful of components."""
    lab = np.full((h, w), bg, np.uint8)
    lab[h // 5:h - h // 5, w // 6:w - w // 6] = fg
    lab[h // 3:h - h // 3, w // 3:w - w // 3] = bg
    lab[h // 2 - h // 12:h // 2 + h // 12, w // 2 - w // 12:w // 2 + w // 12] = fg
    return lab


def variants(case: Case):
    """The five crops of the mixed batch, by name: the case, a plain blob frame, an all-background
    frame, the case flipped left to right, an all-foreground frame."""
    lab = built(case)[0]
    h, w = lab.shape
    return {"case": lab, "plain": plain_frame(h, w, case.fg, case.bg),
            "empty": np.full((h, w), case.bg, np.uint8), "flip": np.ascontiguousarray(lab[:, ::-1]),
            "full": np.full((h, w), case.fg, np.uint8)}


MIXED = ("case", "plain", "empty", "flip", "full")


def expected_variant(case: Case, which: str):
    _, pal, _, min_area, K = built(case)
    return expected((case.name, which), variants(case)[which], pal, min_area, K)


def frames(case: Case, which):
    """[len(which), H, W] uint8 frames holding the named crops top-left, random labels (below
    ``bins``) outside the crop."""
    lab, _, bins, _, _ = built(case)
    h, w = lab.shape
    H, W = h + case.pad[0], w + case.pad[1]
    rng = np.random.default_rng(len(case.name) + 7 * h + w)
    out = rng.integers(0, bins, (len(which), H, W), dtype=np.uint8)
    v = variants(case)
    for i, name in enumerate(which):
        out[i, :h, :w] = v[name]
    return out, (h, w)


# ------------------------------------------------------------------ path conditions
def passing_contours(case: Case) -> int:
    lab, pal, _, min_area, _ = built(case)
    return len(C.component_segments(lab, min_area, pal))


def check_path(case: Case) -> dict:
    """Assert, from the reference alone, the condition that puts the case on its path; returns
    the figures (BASELINE.md lists them)."""
    lab, pal, bins, min_area, K = built(case)
    mask = mask_of(lab, pal)
    total, most = tile_roots(mask)
    fig = {"roots": total, "max_per_tile": most}
    name = case.name
    if name.startswith("rovf_compact"):
        assert most > kTileCap and total <= kMergeCap, fig
        fig["passing"] = passing_contours(case)
        if K == 64 and min_area == 0.0:
            assert fig["passing"] > K, fig
        else:
            assert fig["passing"] <= K, fig
    elif name == "scan_select":
        fig["passing"] = passing_contours(case)
        assert fig["passing"] > kSortCap and total <= kMergeCap and K == K_MAX, fig
    elif name.startswith("fallback_small"):
        assert total > 1.1 * kMergeCap, fig
        node, fg = C.label_components(mask)
        # hole -> foreground -> holes, inside the dense region: a chain of depth >= 4
        w = lab.shape[1]
        depth = 0
        n = int(node[66, 75]) if not fg[66, 75] else int(node[66, 76])
        assert n != 0 and not fg.ravel()[n - 1], "expected a hole of the patch inside the blob's hole"
        while n != 0:
            depth += 1
            y, x = divmod(n - 1, w)
            n = int(node[y, x - 1]) if x > 0 else 0
        fig["depth"] = depth
        assert depth >= 4, fig
    elif name == "tables_full":
        node, _ = C.label_components(mask)
        fig["nodes_per_tile"] = max_nodes_per_tile(node)
        fig["nodes_per_run"] = max_nodes_per_run(node, 256)
        assert fig["nodes_per_tile"] > kHash and fig["nodes_per_run"] > kHash, fig
        assert total <= kMergeCap, fig
    elif name.startswith(("corner_", "tileedge_")):
        where, kind, cy, cx = name.replace("-", "_").split("_")
        cy, cx = int(cy), int(cx)
        assert (cy % TILE == 0) + (cx % TILE == 0) == (2 if where == "corner" else 1)
        node, fg = C.label_components(mask)
        quad = (bool(mask[cy - 1, cx - 1]), bool(mask[cy - 1, cx]), bool(mask[cy, cx - 1]), bool(mask[cy, cx]))
        anti = kind == "anti" or (kind == "bg" and bg_anti(cy, cx))
        want = (False, True, True, False) if anti else (True, False, False, True)
        if kind == "bg":
            want = tuple(not v for v in want)
        assert quad == want, (quad, want)
        nfg = len(np.unique(node[fg]))
        holes = np.unique(node[~fg])
        holes = holes[holes != 0]
        fig["fg"], fig["holes"] = nfg, len(holes)
        if kind == "bg":
            assert nfg == 1 and len(holes) == 2, fig   # the two background regions stay two holes
        else:
            assert nfg == 1 and len(holes) == 0, fig   # one component through the corner contact
    elif name.startswith("thin"):
        assert min(lab.shape) <= 2
    elif name.startswith("edges32"):
        h, w = lab.shape
        assert K == K_MAX and case.pad[0] > 0 and case.pad[1] > 0
        assert (h, w) in EDGE_CROPS
    elif name.startswith("bins"):
        assert bins == int(name.split("-")[1]) and int(lab.max()) < bins
        if bins == 40:
            assert bins > kDenseBins and int(lab.max()) == 39
            assert ((lab == 35) & mask).any() and ((lab == 38) & mask).any()  # both bright classes are foreground
    elif name == "tie":
        node, fg = C.label_components(mask)
        roots = np.unique(node[fg])
        assert len(roots) == 1
        hist = fill_histogram(lab, pal, int(roots[0]), bins)
        fig["hist7"], fig["hist15"] = int(hist[7]), int(hist[15])
        assert hist[7] == hist[15] == hist.max() and hist.sum() == 2 * hist[7], hist
    elif name.startswith("area_edge"):
        a = area_of_rectangle()
        fig["area"] = a
        assert min_area == (a if name.endswith("keep") else np.nextafter(a, np.inf))
        assert passing_contours(case) == (1 if name.endswith("keep") else 0)
    else:
        raise AssertionError(f"no path condition for {name}")
    return fig
