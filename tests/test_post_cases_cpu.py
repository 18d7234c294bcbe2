"""The inputs the device contour statistics are held to in
tests/test_postprocess_topology_gpu.py, checked on the CPU first:

* every case of tests/post_cases.py sits on the path it is listed for, by the reference alone;
* on every case the spec (``components.component_segments``) equals the exact border tracer
  (``reference.segments_exact``), with the case's palette: the spec's validation against the
  hand-checked tracer, extended to exactly these inputs;
* teeth: a spec with the wrong connectivity at the tile-corner cases is rejected.
"""
import numpy as np
import pytest

import post_cases as PC
from semantic_segmentation_server_amd.postprocess import components as C
from semantic_segmentation_server_amd.postprocess import reference as R

IDS = [c.name for c in PC.CASES]


def _rows(segs):
    return [(x[0], round(x[1], 9), x[2], x[3], x[4], x[6]) for x in segs]


@pytest.mark.parametrize("name", IDS)
def test_case_is_on_its_path(name):
    fig = PC.check_path(PC.BY_NAME[name])
    print(f"[post case] {name}: {fig}")


def test_kernel_constants_are_the_sources():
    """The copied constants against the text of csrc/hip/postprocess.hip."""
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                            "csrc", "hip", "postprocess.hip")).read()
    for name in ("kTileCap", "kMergeCap", "kSortCap", "kTSlots", "kMaxDepth", "kAnc", "kPoolPerFrame",
                 "kDenseBins"):
        m = re.search(r"constexpr int %s = (\d+);" % name, src)
        assert m and int(m.group(1)) == getattr(PC, name), name
    assert int(re.search(r"#define SSA_KHASH (\d+)", src).group(1)) == PC.kHash
    assert "constexpr int TW = 32, TH = SSA_CCL_TH;" in src and "#define SSA_CCL_TH 32" in src and PC.TILE == 32


def test_two_tone_mask_is_a_majority_filter():
    rng = np.random.default_rng(3)
    lab = (rng.random((37, 41)) < 0.5).astype(np.uint8)
    pad = np.pad(lab.astype(np.int64), 1, mode="reflect")
    s = sum(pad[dy:dy + 37, dx:dx + 41] for dy in range(3) for dx in range(3))
    assert np.array_equal(PC.mask_of(lab, PC.TWO_TONE), s >= 5)
    cb = PC.checkerboard(70, 75)
    assert np.array_equal(PC.mask_of(cb, PC.TWO_TONE), cb > 0)


def test_tile_roots_counts_tile_local_components():
    cb = PC.checkerboard(64, 64) > 0
    # per full tile: one 8-connected foreground, 512 single background pixels
    assert PC.tile_roots(cb) == (4 * 513, 513)
    solid = np.ones((33, 65), bool)
    assert PC.tile_roots(solid) == (6, 1)
    split = np.zeros((32, 32), bool)
    split[:, 10] = True   # a wall: two background halves
    assert PC.tile_roots(split) == (3, 3)


@pytest.mark.parametrize("name", IDS)
def test_spec_matches_exact_tracer(name):
    case = PC.BY_NAME[name]
    lab, pal, _, min_area, _ = PC.built(case)
    a = _rows(R.segments_exact(lab, min_area, pal))
    b = _rows(C.component_segments(lab, min_area, pal))
    assert a == b, name
    flip = np.ascontiguousarray(lab[:, ::-1])
    assert _rows(R.segments_exact(flip, min_area, pal)) == _rows(C.component_segments(flip, min_area, pal)), name


@pytest.mark.parametrize("name", ["tie", "bins-40", "fallback_small-area4", "thin-2x40"])
def test_mixed_batch_frames_match_exact_tracer(name):
    """The other frames of the GPU file's mixed batch (plain, empty, all foreground)."""
    case = PC.BY_NAME[name]
    _, pal, _, min_area, _ = PC.built(case)
    for which, lab in PC.variants(case).items():
        assert _rows(R.segments_exact(lab, min_area, pal)) == _rows(C.component_segments(lab, min_area, pal)), which


def test_expected_overflow_flag():
    case = PC.BY_NAME["rovf_compact-area0-K64"]
    exp, over = PC.expected_variant(case, "case")
    lab, pal, _, min_area, K = PC.built(case)
    assert over and len(exp) == K
    assert exp == C.component_segments(lab, min_area, pal, max_records=K)
    exp, over = PC.expected_variant(PC.BY_NAME["rovf_compact-area4"], "case")
    assert not over and len(exp) == 1


# ---------------------------------------------------------------- teeth
S8 = np.ones((3, 3), bool)
S4 = np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]], bool)


def label_variant(mask, fg_structure=S8, bg_structure=S4, corner_union=True):
    """``components.label_components`` with the two connectivity structures as parameters
    (plain union-find over the raster). ``corner_union=False`` leaves out the diagonal unions
    that cross a 32x32 tile corner: what a tiled labelling gets when it forgets them."""
    fg = np.asarray(mask).astype(bool)
    h, w = fg.shape
    par = list(range(h * w))

    def find(i):
        while par[i] != i:
            par[i] = par[par[i]]
            i = par[i]
        return i

    for y in range(h):
        for x in range(w):
            st = fg_structure if fg[y, x] else bg_structure
            for dy, dx in ((0, -1), (-1, -1), (-1, 0), (-1, 1)):
                yy, xx = y + dy, x + dx
                if not st[1 + dy][1 + dx] or yy < 0 or xx < 0 or xx >= w or fg[yy, xx] != fg[y, x]:
                    continue
                if not corner_union and dx != 0 and dy != 0 and y % PC.TILE == 0 and max(x, xx) % PC.TILE == 0:
                    continue
                a, b = find(y * w + x), find(yy * w + xx)
                if a != b:
                    par[max(a, b)] = min(a, b)   # the root is the first pixel
    root = np.array([find(i) for i in range(h * w)]).reshape(h, w)
    node = root + 1
    edge = np.zeros((h, w), bool)
    edge[0, :] = edge[-1, :] = edge[:, 0] = edge[:, -1] = True
    outside = np.unique(root[edge & ~fg])
    node[~fg & np.isin(root, outside)] = 0
    return node.astype(np.int64), fg


CORNER_IDS = [n for n in IDS if n.startswith("corner_")]
TILEEDGE_IDS = [n for n in IDS if n.startswith("tileedge_")]


@pytest.mark.parametrize("name", CORNER_IDS + TILEEDGE_IDS)
def test_label_variant_is_the_spec(name):
    lab, pal, _, _, _ = PC.built(PC.BY_NAME[name])
    mask = PC.mask_of(lab, pal)
    a, b = C.label_components(mask), label_variant(mask)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


MUTATIONS = {
    "background joined across the diagonal": (dict(bg_structure=S8), "corner_bg"),
    "corner union dropped": (dict(corner_union=False), ("corner_diag", "corner_anti")),
    "foreground 4-connected": (dict(fg_structure=S4), ("corner_diag", "corner_anti")),
}


@pytest.mark.parametrize("mutation", sorted(MUTATIONS))
def test_wrong_connectivity_is_rejected(mutation, monkeypatch):
    """At each tile corner of the cases it bears on, a spec labelled with the mutated
    connectivity no longer equals the exact tracer; unmutated, the same code path does."""
    kw, prefix = MUTATIONS[mutation]
    names = [n for n in CORNER_IDS if n.startswith(prefix)]
    assert len(names) == (3 if isinstance(prefix, str) else 6)
    for name in names:
        lab, pal, _, min_area, _ = PC.built(PC.BY_NAME[name])
        exact = _rows(R.segments_exact(lab, min_area, pal))
        with monkeypatch.context() as m:
            m.setattr(C, "label_components", label_variant)
            assert _rows(C.component_segments(lab, min_area, pal)) == exact, name
        with monkeypatch.context() as m:
            m.setattr(C, "label_components", lambda mask: label_variant(mask, **kw))
            assert _rows(C.component_segments(lab, min_area, pal)) != exact, (mutation, name)
