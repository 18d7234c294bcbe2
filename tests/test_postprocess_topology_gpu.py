"""The device contour statistics (csrc/hip/postprocess.hip) against the spec
(``components.component_segments``) on the adversarial small inputs of tests/post_cases.py:
crowded tiles on the compact merge (rovf list), raster-scan selection, the union-find fallback
with nested holes, full LDS accumulation tables, contacts across tile corners, thin crops, crop
sizes around the tile, class-bin counts, K = 256, ties, the area threshold, and state carried
between calls on one object. tests/test_post_cases_cpu.py holds the spec to the exact tracer
on the same inputs and asserts that each case is on the path it is listed for.

One comparator everywhere: the record count, its sign (negative: more than K contours passed),
then label, score, area, cx, cy of every record exactly. The score is compared as
``np.float32(score)``: the device computes ``(float)((double)h[best] / (double)tot)`` and the
spec the same double quotient of the same integers, so the float32 roundings are equal.
Words of the record buffer past ``1 + 5 n`` are not asserted: the kernel does not define them.
"""
import numpy as np
import pytest
import torch

import post_cases as PC

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = -12345.0
POISON = 31337.0


@pytest.fixture
def accum(request, monkeypatch):
    """The accumulation pass (1: 32x32 tiles, 2: 64x64 tiles, 0: strips), as the existing
    ``post_accum`` fixture of tests/test_hip_kernels.py sets it."""
    monkeypatch.setenv("SSA_POST_ACCUM", str(request.param))
    return request.param


ACCUMS = (1, 2, 0)
ACCUM_ID = {1: "tiles", 2: "tiles64", 0: "strips"}
ALL_ACCUM = pytest.mark.parametrize("accum", ACCUMS, indirect=True, ids=[ACCUM_ID[a] for a in ACCUMS])


def _post(H, W, pal, K, bins):
    from semantic_segmentation_server_amd.postprocess.device import DevicePostprocess
    return DevicePostprocess(torch.device(DEV), H, W, pal, K=K, bins=bins)


def _run(post, maps, crop, min_area):
    """One call through a record buffer with a guard row before and after -> [B, 1 + 5K]."""
    B = maps.shape[0]
    h, w = crop
    raw = torch.full((B + 2, 1 + 5 * post.K), GUARD, dtype=torch.float32, device=DEV)
    raw[1:B + 1] = POISON
    out = raw[1:B + 1]
    post.run(torch.from_numpy(np.ascontiguousarray(maps)).to(DEV), w, h, min_area, out=out)
    torch.cuda.synchronize()
    r = raw.cpu().numpy()
    assert (r[0] == GUARD).all() and (r[-1] == GUARD).all(), "guard rows written"
    return r[1:B + 1]


def assert_records(row, exp, over, W, H, what):
    """THE comparator: count, sign of the count, five fields of every record, exact."""
    c = row[0]
    assert not np.isnan(c), (what, "no records: root pool exhausted")
    n = abs(int(c))
    assert c == np.float32(int(c)) and n == len(exp), (what, float(c), len(exp))
    assert (c < 0) == bool(over), (what, float(c), over)
    got = row[1:1 + 5 * n].reshape(n, 5)
    for j in range(n):
        lab, score, area, cx, cy = exp[j][:5]
        assert got[j, 0] == np.float32(int(lab)), (what, j, got[j], exp[j])
        assert got[j, 1] == np.float32(score), (what, j, got[j], exp[j])
        assert got[j, 2] == np.float32(min(1.0, area / (W * H))), (what, j, got[j], exp[j])
        assert got[j, 3] == np.float32(min(1.0, cx / W)), (what, j, got[j], exp[j])
        assert got[j, 4] == np.float32(min(1.0, cy / H)), (what, j, got[j], exp[j])
    return n


def _defined(rec):
    """The defined words of every row: the count and the 5 n record words."""
    return [row[:1 + 5 * abs(int(row[0]))].copy() for row in rec]


def _check_case(case, which, post=None):
    lab, pal, bins, min_area, K = PC.built(case)
    maps, crop = PC.frames(case, which)
    H, W = maps.shape[1:]
    post = post or _post(H, W, pal, K, bins)
    rec = _run(post, maps, crop, min_area)
    for i, name in enumerate(which):
        exp, over = PC.expected_variant(case, name)
        assert_records(rec[i], exp, over, W, H, (case.name, name, i))
    return rec


CASE_PARAMS = [pytest.param(c.name, a, id=f"{c.name}-{ACCUM_ID[a]}")
               for c in PC.CASES for a in ((1,) if c.any_accum else ACCUMS)]


@pytest.mark.parametrize("name,accum", CASE_PARAMS, indirect=["accum"])
def test_case_alone_and_in_a_mixed_batch(name, accum):
    """Every case at B = 1, and at B = 5 beside a plain blob frame, an all-background frame, its
    own mirror image and an all-foreground frame: fallback and compact frames, crowded and
    empty ones, side by side in one root pool."""
    case = PC.BY_NAME[name]
    _check_case(case, ("case",))
    _check_case(case, PC.MIXED)


def test_more_than_32_bins_take_the_strips_whatever_accum(monkeypatch):
    """bins = 40 does not fit the tile kernels' dense class counters: every ``accum`` value runs
    the strip kernel and gives the same words."""
    case = PC.BY_NAME["bins-40"]
    recs = []
    for a in ACCUMS:
        monkeypatch.setenv("SSA_POST_ACCUM", str(a))
        recs.append(_defined(_check_case(case, PC.MIXED)))
    for r in recs[1:]:
        assert all(np.array_equal(x, y) for x, y in zip(r, recs[0]))


# ---------------------------------------------------------------- state carried between calls
def _embed(crops, H, W, bins, seed):
    rng = np.random.default_rng(seed)
    out = rng.integers(0, bins, (len(crops), H, W), dtype=np.uint8)
    for i, c in enumerate(crops):
        out[i, :c.shape[0], :c.shape[1]] = c
    return out


def _check_crops(post, key, crops, min_area, seed=0):
    """Run the crops (all of one size) top-left in the object's frame; each against the spec."""
    pal = post.palette.cpu().numpy()
    maps = _embed(crops, post.H, post.W, post.bins, seed)
    rec = _run(post, maps, crops[0].shape, min_area)
    for i, c in enumerate(crops):
        exp, over = PC.expected((key, i, min_area, post.K), c, pal, min_area, post.K)
        assert_records(rec[i], exp, over, post.W, post.H, (key, i, min_area))
    return rec


@ALL_ACCUM
def test_fallback_then_plain_then_crowded_on_one_object(accum):
    """One object, one B: a union-find fallback frame, a plain one, the fallback frame mirrored,
    then the crowded compact frame at a smaller crop. ``k_ccl_merge`` re-zeroes ``flag[2]`` and
    ``flag[4]`` for the next call and ``nslot``, the pool, ``rlist``, ``rpar`` and ``cidx`` are
    reused: a stale value of any of them shows as a wrong record here."""
    fb = PC.fallback_labels()
    rovf = PC.checkerboard(70, 75)
    plain = PC.plain_frame(PC.FB_H, PC.FB_W, 1, 0)
    flip = np.ascontiguousarray(fb[:, ::-1])
    assert PC.tile_roots(fb > 0)[0] > PC.kMergeCap >= PC.tile_roots(rovf > 0)[0]
    post = _post(PC.FB_H, PC.FB_W, PC.TWO_TONE, PC.K_MAX, 2)
    _check_crops(post, "seq-fb", [fb, plain], 0.0)
    _check_crops(post, "seq-plain", [plain, plain[::-1].copy()], 0.0)
    _check_crops(post, "seq-flip", [flip, fb], 4.0)
    _check_crops(post, "seq-rovf", [rovf, np.ascontiguousarray(rovf[:, ::-1])], 0.0, seed=1)
    _check_crops(post, "seq-rovf", [rovf, np.ascontiguousarray(rovf[:, ::-1])], 4.0, seed=2)
    _check_crops(post, "seq-fb", [fb, plain], 0.0)


@ALL_ACCUM
def test_pool_exhausted_then_fitting_on_one_object(accum):
    """B copies of ``fallback_small`` reserve B * R pool entries (R: the frame's tile-local
    roots) against P = max(B * 8192, N + 1) + N / 2 + 1: at B = 4 three frames fit and one does
    not. The frame that did not fit comes back NaN (which one is up to the order of the
    reservations), the others are exact, and a fitting batch on the same object right after is
    exact in every frame."""
    fb = PC.fallback_labels()
    plain = PC.plain_frame(PC.FB_H, PC.FB_W, 1, 0)
    B = 4
    N = PC.FB_H * PC.FB_W
    R = PC.tile_roots(fb > 0)[0]
    P = max(B * PC.kPoolPerFrame, N + 1) + N // 2 + 1
    assert R > PC.kMergeCap and 3 * R <= P < 4 * R, (R, P)
    post = _post(PC.FB_H, PC.FB_W, PC.TWO_TONE, 64, 2)
    exp, over = PC.expected(("pool", 4.0), fb, PC.TWO_TONE, 4.0, 64)
    for _ in range(2):
        rec = _run(post, np.stack([fb] * B), fb.shape, 4.0)
        nan = np.isnan(rec[:, 0])
        assert int(nan.sum()) == B - P // R == 1, rec[:, 0]
        for i in np.nonzero(~nan)[0]:
            assert_records(rec[i], exp, over, PC.FB_W, PC.FB_H, ("pool", int(i)))
        _check_crops(post, "pool-fit", [plain, fb, np.ascontiguousarray(fb[:, ::-1]), plain], 4.0)


@ALL_ACCUM
def test_crop_change_on_one_object(accum):
    """Crop (97, 131), then (33, 32), then (97, 131) again, inside one frame size on one object:
    the tile grid, the edge lines and the per-pixel arrays' row stride all change."""
    case = PC.BY_NAME["edges32-p0.6-97x131"]
    lab, pal, bins, min_area, K = PC.built(case)
    H, W = lab.shape[0] + 5, lab.shape[1] + 7
    post = _post(H, W, pal, K, bins)
    big = [lab, np.ascontiguousarray(lab[:, ::-1])]
    small = [np.ascontiguousarray(c[:33, :32]) for c in big]
    _check_crops(post, "crop-big", big, min_area)
    _check_crops(post, "crop-small", small, min_area, seed=3)
    _check_crops(post, "crop-big", big, min_area, seed=4)


@pytest.mark.parametrize("name", ["scan_select", "fallback_small-area0-K256", "edges32-p0.6-97x131"])
@ALL_ACCUM
def test_three_repeats_bit_identical(name, accum):
    """The same mixed batch three times on one object: the defined words are bit-identical
    (and equal to the spec's)."""
    case = PC.BY_NAME[name]
    lab, pal, bins, _, K = PC.built(case)
    post = _post(lab.shape[0] + case.pad[0], lab.shape[1] + case.pad[1], pal, K, bins)
    outs = [_defined(_check_case(case, PC.MIXED, post)) for _ in range(3)]
    for o in outs[1:]:
        assert all(x.tobytes() == y.tobytes() for x, y in zip(o, outs[0]))
