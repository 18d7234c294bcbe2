"""The inputs the device class-region kernels are held to in tests/test_regions_paths_gpu.py,
checked on the CPU first:

* every case of tests/region_cases.py has the property it is listed for, by the reference's
  root plane and the geometry alone;
* a second oracle that shares nothing with the definition (a plain queue flood fill over the
  8 neighbours) gives, packed, the words of ``regions.encode`` on every case, ``sum_conf``
  included, and on the exhaustive windows: all 4096 fillings at the tile corner, every 16th
  elsewhere;
* teeth: the same flood fill over 4 neighbours is rejected at every window position and at
  the two fillings that are linked across the tile corner alone.
"""
import os
import re

import numpy as np
import pytest

import region_cases as RC
from semantic_segmentation_server_amd.postprocess import regions as RG

IDS = [c.name for c in RC.CASES]


def test_constants_are_the_sources():
    """The two constants hip_ops does not export, against the text of the kernel file."""
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                            "csrc", "hip", "class_regions.hip")).read()
    for name, value in (("kBuckets", RC.BUCKETS), ("kSelThreads", RC.SELECT_THREADS), ("kTile", RC.TW),
                        ("kCandidates", RC.CAND), ("kMaxK", RC.KMAX)):
        m = re.search(r"constexpr int %s = (\d+);" % name, src)
        assert m and int(m.group(1)) == value, name
    assert RC.TW == RC.TH and RC.TH % 2 == 0


@pytest.mark.parametrize("name", IDS)
def test_case_has_its_property(name):
    case = RC.BY_NAME[name]
    fig = case.check(RC.built(case))
    print(f"[region case] {name}: {fig}")


@pytest.mark.parametrize("name", IDS)
def test_flood_fill_packs_to_the_definition(name):
    case = RC.BY_NAME[name]
    b = RC.built(case)
    for with_conf in (False, True):
        want = RC.want(case, with_conf)
        for i, lab in enumerate(b.labels):
            got = RC.flood_encode(lab, b.crop_w, b.crop_h, b.classes, b.min_pixels, b.K,
                                  b.conf[i] if with_conf else None)
            assert np.array_equal(got, want[i]), (name, with_conf, i, np.flatnonzero(got != want[i])[:8])


def test_limit_shapes_pass_the_geometry_check_and_one_more_pixel_does_not():
    mp = RC.least_min_pixels(RC.LIMIT)
    RG.check_geometry(RC.LIMIT, 1, mp, RC.KMAX)
    RG.check_geometry(1, RC.LIMIT, mp, RC.KMAX)
    assert RC.LIMIT * RC.LIMIT < 1 << 32
    for cw, ch in ((RC.LIMIT + 1, 1), (1, RC.LIMIT + 1)):
        with pytest.raises(ValueError):
            RG.check_geometry(cw, ch, RC.least_min_pixels(RC.LIMIT + 1), RC.KMAX)
    with pytest.raises(ValueError):  # one candidate too many
        RG.check_geometry(RC.LIMIT, 1, mp - 1, RC.KMAX)


# ---------------------------------------------------------------- the exhaustive windows
def test_window_geometry():
    ch, cw = RC.WIN_CROP
    assert (ch, cw) == (RC.TH + 3, RC.TW + 4) and RC.WIN_MAP == (ch + 2, cw + 2)
    assert RC.WIN_BATCH <= 256 and RC.WIN_BATCHES * RC.WIN_BATCH == RC.WIN_FILLINGS == 4096
    ya, xa = RC.WIN_POS["a"]
    assert ya == 1 and xa + RC.WIN_W < RC.TW                       # rows 1|2: two waves, 2|3: one
    yb, xb = RC.WIN_POS["b"]
    assert (yb, xb) == (10, RC.TW - 2)
    assert RC.WIN_POS["c"] == (RC.TH - 1, 5) and RC.WIN_POS["d"] == (RC.TH - 1, RC.TW - 2)
    ye, xe = RC.WIN_POS["e"]
    assert ye < ch < ye + RC.WIN_H <= RC.WIN_MAP[0] and xe < cw < xe + RC.WIN_W <= RC.WIN_MAP[1]
    lab = RC.window_frame("e", 0)
    assert (lab[ye:ye + RC.WIN_H, xe:xe + RC.WIN_W] == 1).all() and int((lab > 0).sum()) == 12
    RG.check_geometry(cw, ch, 1, RC.WIN_K)
    assert set(RC.WIN_PATH) == set(RC.WIN_POS)


def _window_against_definition(pos, fillings):
    """Flood fill on the 12 cells == regions.encode of the whole frame, both forms. Returns the
    largest n_regions met."""
    ch, cw = RC.WIN_CROP
    most = 0
    for j in range(RC.WIN_BATCHES):
        mine = [f for f in fillings if f // RC.WIN_BATCH == j]
        if not mine:
            continue
        labels, conf = RC.window_batch(pos, j)
        for with_conf in (False, True):
            want = RC.window_want(pos, j, with_conf)
            rw = RG.words_per_region(with_conf)
            for f in mine:
                b = f % RC.WIN_BATCH
                ref = RG.encode(labels[b], cw, ch, RC.WIN_CLASSES, 1, RC.WIN_K,
                                out=np.full(4 + rw * RC.WIN_K, RC.SENT, np.uint32),
                                conf=conf[b] if with_conf else None)
                assert np.array_equal(want[b], ref), (pos, f, with_conf)
                most = max(most, int(ref[0]))
    return most


# one filling of every 16; its low four bits (the first row of the window) take every value beside every
# value of the next four
SAMPLE = [16 * i + (i + i // 16) % 16 for i in range(RC.WIN_FILLINGS // 16)]


def test_every_filling_at_the_corner_matches_the_definition():
    most = _window_against_definition("d", range(RC.WIN_FILLINGS))
    assert 4 <= most <= RC.WIN_K  # every region of every filling has a record


@pytest.mark.parametrize("pos", [p for p in sorted(RC.WIN_POS) if p != "d"])
def test_every_16th_filling_matches_the_definition(pos):
    assert _window_against_definition(pos, SAMPLE) <= RC.WIN_K


def _cells(*cells):
    """The filling with class 2 in the given (row, column) cells and class 1 in the others."""
    f = 0
    for r, c in cells:
        f |= 1 << (r * RC.WIN_W + c)
    return f


# class 2 in two cells that touch only across the tile corner (window rows 0|1, columns 1|2),
# class 1 in the other ten
CORNER_LINKS = {"diagonal": _cells((0, 1), (1, 2)), "anti-diagonal": _cells((0, 2), (1, 1))}


@pytest.mark.parametrize("which", sorted(CORNER_LINKS))
def test_four_connectivity_is_rejected_at_the_corner(which):
    ch, cw = RC.WIN_CROP
    f = CORNER_LINKS[which]
    lab = RC.window_frame("d", f)
    y0, x0 = RC.WIN_POS["d"]
    assert y0 + 1 == RC.TH and x0 + 2 == RC.TW
    ref = RG.encode(lab, cw, ch, RC.WIN_CLASSES, 1, RC.WIN_K)
    two = RG.decode(ref)
    two = two[two["label"] == 2]
    assert len(two) == 1 and two[0]["pixels"] == 2          # one region through the corner
    assert np.array_equal(RC.flood_encode(lab, cw, ch, RC.WIN_CLASSES, 1, RC.WIN_K, fill=0), ref)
    four = RC.flood_encode(lab, cw, ch, RC.WIN_CLASSES, 1, RC.WIN_K, fill=0, neighbours=RC.N4)
    assert not np.array_equal(four, ref) and four[0] == ref[0] + 1


@pytest.mark.parametrize("pos", sorted(RC.WIN_POS))
def test_four_connectivity_is_rejected_by_the_windows(pos):
    ch, cw = RC.WIN_CROP
    win = RC.WIN_POS[pos] + (RC.WIN_H, RC.WIN_W)
    wrong = 0
    for f in SAMPLE:
        j, b = divmod(f, RC.WIN_BATCH)
        lab = RC.window_frame(pos, f)
        four = RC.flood_encode(lab, cw, ch, RC.WIN_CLASSES, 1, RC.WIN_K, neighbours=RC.N4, window=win)
        wrong += not np.array_equal(four, RC.window_want(pos, j, False)[b])
    assert wrong > 0, pos
    print(f"[region windows] {pos}: 4-connectivity differs on {wrong} of {len(SAMPLE)} fillings")


@pytest.mark.parametrize("name", ["shape-%dx%d" % RC.SHAPES[-1], "stats-conf-runs"])
def test_four_connectivity_is_rejected_by_cases(name):
    case = RC.BY_NAME[name]
    b = RC.built(case)
    four = RC.flood_encode(b.labels[0], b.crop_w, b.crop_h, b.classes, b.min_pixels, b.K, b.conf[0],
                           neighbours=RC.N4)
    assert not np.array_equal(four, RC.want(case, True)[0])
