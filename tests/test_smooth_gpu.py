"""Device label smoothing (csrc/hip/label_smooth.hip) against the numpy definition
(postprocess/smooth.py), and the chain / engine layers that run it first.

Every comparison is exact. The outputs are views of exactly B * H * W bytes at the head of larger
buffers, prefilled with a sentinel (every byte must be written) and followed by a sentinel tail
that must come back unchanged; the inputs must come back unchanged.
"""
import functools

import numpy as np
import pytest
import torch

from semantic_segmentation_server_amd.postprocess import mask_rle as MR
from semantic_segmentation_server_amd.postprocess import regions as RG
from semantic_segmentation_server_amd.postprocess import smooth as SM
from semantic_segmentation_server_amd.postprocess import stable as SB

import chip_poison as CP
import smooth_cases as SC
import stable_cases as STC

pytestmark = pytest.mark.gpu

DEV = "cuda"
TAIL, TAIL_SENT, OUT_SENT = 256, 0xA5, 0xEE


def _hip():
    from semantic_segmentation_server_amd.ops import hip_ops
    return hip_ops


def _out_plane(shape):
    """(a sentinel-filled view of the head of a larger buffer, the buffer)."""
    n = int(np.prod(shape))
    buf = torch.full((n + TAIL,), OUT_SENT, dtype=torch.uint8, device=DEV)
    buf[n:] = TAIL_SENT
    return buf[:n].view(*shape), buf


def _device(labels, conf, ch, cw, R):
    """One launch over the batch -> (labels, codes or None) as numpy."""
    hip = _hip()
    B, H, W = labels.shape
    li = torch.from_numpy(np.array(labels)).to(DEV)  # a writable copy: the cases are read-only
    ci = None if conf is None else torch.from_numpy(np.array(conf)).to(DEV)
    lo, lbuf = _out_plane(labels.shape)
    co, cbuf = _out_plane(labels.shape) if ci is not None else (None, None)
    hip.label_smooth(li, lo, ci, co, B=B, H=H, W=W, crop_h=ch, crop_w=cw, R=R)
    torch.cuda.synchronize()
    assert np.array_equal(li.cpu().numpy(), labels)
    assert ci is None or np.array_equal(ci.cpu().numpy(), conf)
    for buf in (lbuf, cbuf):
        assert buf is None or bool((buf[B * H * W:] == TAIL_SENT).all())
    return lo.cpu().numpy(), (None if co is None else co.cpu().numpy())


def _same(got, want):
    assert np.array_equal(got[0], want[0])
    assert (got[1] is None) == (want[1] is None)
    assert got[1] is None or np.array_equal(got[1], want[1])


def _check(lab, codes, ch, cw, R, must_change=True):
    """Device == oracle with and without the conf plane; the pad pixels separately."""
    B, H, W = lab.shape
    want = SM.apply(lab, codes, cw, ch, R)
    if must_change:
        assert (want[0] != lab).any()  # from the oracle: the case is not vacuous
    pad = np.ones((H, W), bool)
    pad[:ch, :cw] = False
    for cf in (codes, None):
        got = _device(lab, cf, ch, cw, R)
        _same(got, (want[0], None if cf is None else want[1]))
        assert np.array_equal(got[0][:, pad], lab[:, pad])
        assert cf is None or np.array_equal(got[1][:, pad], cf[:, pad])
    return want


# ---- every three-label 3 x 3 pattern ------------------------------------------------------------

@pytest.mark.parametrize("conf", [False, True])
def test_every_three_label_3x3_pattern_in_one_launch(conf):
    lab, codes = SC.exhaustive()  # B = 19683 in grid z
    want_c, kept, _, _ = SC.exhaustive_centres()
    want = SM.apply(lab, codes if conf else None, 3, 3, 1)
    got = _device(lab, codes if conf else None, 3, 3, 1)
    _same(got, want)
    assert np.array_equal(got[0][:, 1, 1], want_c) and int(kept.sum()) == 11811


# ---- geometry -----------------------------------------------------------------------------------

GEOMETRIES = ["cpu0", "cpu1", "cpu2", "cpu3", "cpu4", "one_wider", "one_narrower", "one_taller",
              "one_shorter", "edge_on_tile_edge"]


@pytest.mark.parametrize("R", [1, 2, 3])
@pytest.mark.parametrize("name", GEOMETRIES)
def test_geometries(name, R):
    tw, th = _hip().label_smooth_tile()
    geo = SC.gpu_geometries(tw, th)
    assert sorted(geo) == sorted(GEOMETRIES)
    H, W, ch, cw = geo[name]
    lab, codes = SC.speckled(200 + GEOMETRIES.index(name), 2, H, W)
    _check(lab, codes, ch, cw, R, must_change=ch * cw > 1)  # a 1 x 1 crop has nothing to outvote


@pytest.mark.parametrize("R", [1, 2, 3])
def test_a_crop_smaller_than_the_window(R):
    lab, codes = SC.below_window()
    want = _check(lab, codes, 2, 2, R)
    assert want[0][0, :2, :2].tolist() == [[3, 3], [3, 3]]


@pytest.mark.parametrize("R", [1, 2, 3])
def test_a_speckle_cluster_cut_by_the_edge_between_two_tiles(R):
    tw, _ = _hip().label_smooth_tile()
    lab, codes = SC.cut_cluster(tw)
    want = _check(lab, codes, 12, 2 * tw, R)
    assert (want[0][0, 3:8, tw - 3:tw + 3] != lab[0, 3:8, tw - 3:tw + 3]).any()


# ---- the uniform-tile path ----------------------------------------------------------------------

@pytest.mark.parametrize("R", [1, 3])
def test_a_uniform_tile_beside_a_tile_with_one_odd_pixel_on_the_shared_edge(R):
    tw, th = _hip().label_smooth_tile()
    # three tiles in a row: the first uniform with its halo, the second uniform but for the odd
    # pixel its halo sees, the third holds that pixel in its first column
    lab = np.full((1, 8, 3 * tw), 5, np.uint8)
    lab[0, 4, 2 * tw] = 9
    codes = np.random.default_rng(3).integers(0, 256, lab.shape).astype(np.uint8)
    want = _check(lab, codes, 8, 3 * tw, R)
    assert (want[0] == 5).all()  # outvoted
    near = (slice(0, 1), slice(3, 6), slice(2 * tw - 1, 2 * tw))  # its neighbours in the second tile
    assert (want[0][near] == 5).all() and np.array_equal(want[1][near], codes[near])
    win = codes[0, 4 - R:5 + R, 2 * tw - R:2 * tw + R + 1].astype(np.int64)
    assert want[1][0, 4, 2 * tw] == (win.sum() - codes[0, 4, 2 * tw]) // (win.size - 1)


def test_a_tile_uniform_in_itself_whose_corner_is_outvoted_by_its_halo():
    tw, th = _hip().label_smooth_tile()
    lab = np.full((1, 2 * th, 2 * tw), 9, np.uint8)
    lab[0, :th, :tw] = 5
    codes = np.random.default_rng(4).integers(0, 256, lab.shape).astype(np.uint8)
    want = _check(lab, codes, 2 * th, 2 * tw, 1)
    assert want[0][0, th - 1, tw - 1] == 9 and int((want[0] != lab).sum()) == 1


# ---- batch --------------------------------------------------------------------------------------

def test_five_frames_in_one_launch_equal_five_launches():
    lab, codes = SC.speckled(300, 5, 33, 70)
    ch, cw = 31, 67
    once = _device(lab, codes, ch, cw, 2)
    each = [_device(lab[b:b + 1], codes[b:b + 1], ch, cw, 2) for b in range(5)]
    _same(once, (np.concatenate([e[0] for e in each]), np.concatenate([e[1] for e in each])))
    _same(once, SM.apply(lab, codes, cw, ch, 2))
    assert len({once[0][b].tobytes() for b in range(5)}) == 5


# ---- wrapper refusals ---------------------------------------------------------------------------

def test_wrapper_refusals_name_the_argument():
    hip = _hip()
    B, H, W, ch, cw = 2, 6, 7, 5, 6
    n = B * H * W
    lab = torch.zeros((B, H, W), dtype=torch.uint8, device=DEV)
    cf = torch.zeros_like(lab)
    big = torch.full((4 * n,), OUT_SENT, dtype=torch.uint8, device=DEV)
    lo, co = big[:n].view(B, H, W), big[2 * n:3 * n].view(B, H, W)
    kw = dict(B=B, H=H, W=W, crop_h=ch, crop_w=cw, R=1)

    def bad(match, exc=ValueError, args=None, **over):
        a = dict(labels_in=lab, labels_out=lo, conf_in=cf, conf_out=co)
        a.update(args or {})
        with pytest.raises(exc, match=match):
            hip.label_smooth(a["labels_in"], a["labels_out"], a["conf_in"], a["conf_out"], **{**kw, **over})

    bad("labels_in", TypeError, args=dict(labels_in=lab.to(torch.int32)))
    bad("conf_out", TypeError, args=dict(conf_out=co.to(torch.int16)))
    bad("labels_out: shape", args=dict(labels_out=torch.zeros((B, H, W + 1), dtype=torch.uint8, device=DEV)))
    bad("conf_in: shape", args=dict(conf_in=torch.zeros((B + 1, H, W), dtype=torch.uint8, device=DEV)))
    bad("R 0 outside", R=0)
    bad("R 4 outside", R=4)
    bad("crop", crop_w=W + 1)
    bad("crop", crop_h=0)
    bad("both given or both None", args=dict(conf_out=None))
    bad("both given or both None", args=dict(conf_in=None))
    # a plane on another device: with one GPU the only other device is the host, and a host tensor
    # is refused by the wrapper's per-plane check ("must be a CUDA tensor") before its comparison
    # of the planes' devices, which needs two GPUs and is not reached by this suite
    bad("labels_out: must be a CUDA tensor", args=dict(labels_out=torch.zeros((B, H, W), dtype=torch.uint8)))
    bad("labels_in and labels_out overlap", args=dict(labels_out=lab))  # out is in
    bad("conf_in and conf_out overlap", args=dict(conf_out=cf))
    bad("labels_in and conf_in overlap", args=dict(conf_in=lab))
    bad("labels_out and conf_out overlap", args=dict(conf_out=lo))
    bad("labels_out and conf_out overlap", args=dict(conf_out=big[n // 2:n // 2 + n].view(B, H, W)))
    torch.cuda.synchronize()
    assert bool((big == OUT_SENT).all())  # nothing was launched


# ---- the chain, eager and captured ---------------------------------------------------------------

CH_H = CH_W = 33
CROP_H, CROP_W = 33, 31
CLS, KS, CAP = tuple(range(1, 8)), 16, 1100


def _chain_maps(T):
    lab, code = STC.flicker(41, T, CH_H, CH_W, flip=0.1, block=5)
    return (lab % 8).astype(np.uint8), code


def _chain(conf, R, N):
    from semantic_segmentation_server_amd.postprocess.device import DevicePostprocess
    kw = dict(stable_frames=N, stable_gate=90 if conf else 0, stable_streams=1) if N else {}
    return DevicePostprocess(torch.device(DEV), CH_H, CH_W, np.zeros((256, 3), np.int32), K=8, bins=8,
                             mask_cap=CAP, region_cap=KS, region_classes=RG.class_mask(CLS),
                             region_min_pixels=3, region_conf=conf, smooth_radius=R, **kw)


def _chain_want(lab, code, conf, R, N):
    """The host chain: smooth.apply -> Stabilizers.step -> MR.encode / RG.encode, per frame."""
    st = SB.Stabilizers(N, 90 if conf else 0) if N else None
    rw = 7 if conf else 6
    out = []
    for t in range(len(lab)):
        l, c = SM.apply(lab[t:t + 1], code[t:t + 1] if conf else None, CROP_W, CROP_H, R)
        if st is not None:
            l, c = st.step(l, c, CROP_W, CROP_H, [0])
        out.append((l[0], None if c is None else c[0], MR.encode(l[0], CROP_W, CROP_H, CAP),
                    RG.encode(l[0], CROP_W, CROP_H, RG.class_mask(CLS), 3, KS,
                              out=np.zeros(4 + rw * KS, np.uint32), **({"conf": c[0]} if conf else {}))))
    return out


def _chain_check(dp, lab_t, cf_t, want, conf):
    l, c, mask, reg = want
    assert np.array_equal(lab_t[0].cpu().numpy(), l)
    if conf:
        assert np.array_equal(cf_t[0].cpu().numpy(), c)
    m = dp.fetch_masks(dp.last_mask)[0]
    assert np.array_equal(m[:MR.used_words(mask)], mask[:MR.used_words(mask)])
    r = dp.fetch_regions(dp.last_regions)[0]
    u = RG.used_words(reg, KS, conf=conf)
    assert np.array_equal(r[:u], reg[:u])


@pytest.mark.parametrize("R,N", [(1, 3), (2, 0)])
@pytest.mark.parametrize("conf", [False, True])
def test_chain_eager_and_captured_equal_the_host_chain(conf, R, N):
    lab, code = _chain_maps(5)
    want = _chain_want(lab, code, conf, R, N)
    smooth_only = _chain_want(lab, code, conf, R, 0)
    assert any((w[0] != lab[t]).any() for t, w in enumerate(smooth_only))
    assert not N or any((w[0] != s[0]).any() for w, s in zip(want, smooth_only))  # both stages bite
    dp = _chain(conf, R, N)
    lab_t = torch.zeros((1, CH_H, CH_W), dtype=torch.uint8, device=DEV)
    cf_t = torch.zeros_like(lab_t) if conf else None

    def load(t):
        lab_t.copy_(torch.from_numpy(lab[t:t + 1]))
        if conf:
            cf_t.copy_(torch.from_numpy(code[t:t + 1]))

    for t in range(5):  # eager
        load(t)
        dp.run(lab_t, CROP_W, CROP_H, 4.0, conf=cf_t)
        _chain_check(dp, lab_t, cf_t, want[t], conf)
    assert set(dp._smooth_bufs) == {(1, conf)}  # one scratch label plane, a code plane with conf
    assert (dp._smooth_bufs[(1, conf)][1] is not None) == conf
    dp.reset_tracks()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        load(0)
        dp.run(lab_t, CROP_W, CROP_H, 4.0, conf=cf_t)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        dp.run(lab_t, CROP_W, CROP_H, 4.0, conf=cf_t)
    dp.reset_tracks()  # the warm-up run advanced the state
    for t in range(5):  # replayed
        load(t)
        g.replay()
        _chain_check(dp, lab_t, cf_t, want[t], conf)


def test_flag_off_makes_no_buffer_and_no_launch():
    from semantic_segmentation_server_amd.postprocess.device import DevicePostprocess
    dp = DevicePostprocess(torch.device(DEV), CH_H, CH_W, np.zeros((256, 3), np.int32), K=8, bins=8,
                           mask_cap=CAP)
    lab, _ = _chain_maps(1)
    lab_t = torch.from_numpy(lab[:1].copy()).to(DEV)
    dp.run(lab_t, CROP_W, CROP_H, 4.0)
    torch.cuda.synchronize()
    assert dp.smooth_radius == 0 and not dp._smooth_bufs
    assert np.array_equal(lab_t.cpu().numpy(), lab[:1])


# ---- engine with graphs -------------------------------------------------------------------------

def _cfg(**kw):
    from semantic_segmentation_server_amd import config as C
    base = dict(input_size=129, batch=1, streams=1, backend="hip", graph=True, min_area_ratio=0.0005,
                serve_masks=True, serve_regions=True, region_min_area_ratio=0.001, smooth_labels=1)
    base.update(kw)
    return C.Config(**base)


@functools.lru_cache(maxsize=None)
def _frames():
    from semantic_segmentation_server_amd.runtime.sources import SyntheticSource
    src = SyntheticSource(160, 120, pool=2, seed=11)
    return [src.read_batch(1)[0].copy() for _ in range(2)]


@pytest.mark.parametrize("mode", ["fast", "exact"])  # the device chain; the host path
def test_engine_with_graphs_serves_the_smoothed_maps(mode):
    from semantic_segmentation_server_amd.runtime.engine import Engine
    eng = Engine(_cfg(contour_mode=mode), torch.device(DEV))
    assert eng.smooth_radius == 1
    eng.set_camera(160, 120)
    cw, ch = eng.crop_w, eng.crop_h
    for k, f in enumerate(_frames()):
        raw = eng._infer_eager(torch.from_numpy(f).to(DEV)).cpu().numpy()
        sm, _ = SM.apply(raw, None, cw, ch, 1)
        eng.step(f, [k], [0.0], 0)
        want = MR.encode(sm[0], cw, ch, eng.mask_cap)
        u = MR.used_words(want)
        assert np.array_equal(eng.masks[0][:u], want[:u]), k
        want = RG.encode(sm[0], cw, ch, eng.region_mask, eng.region_min_pixels, eng.region_cap)
        u = RG.used_words(want, eng.region_cap)
        assert np.array_equal(eng.regions[0][:u], want[:u]), k
        assert np.array_equal(eng._static["labels"][0].cpu().numpy(), sm[0]), k  # pad rows: the raw map's
    assert (eng._hip_post is not None and bool(eng._hip_post._smooth_bufs)) == (mode == "fast")


# ---- poison -------------------------------------------------------------------------------------

def test_poisoned_lds_and_registers_do_not_change_the_result():
    CP.require()
    hip = _hip()
    tw, th = hip.label_smooth_tile()
    H, W, ch, cw = SC.gpu_geometries(tw, th)["edge_on_tile_edge"]
    lab, codes = SC.speckled(209, 2, H, W)
    li, ci = torch.from_numpy(lab).to(DEV), torch.from_numpy(codes).to(DEV)

    def run(poisoned):
        lo, co = torch.full_like(li, OUT_SENT), torch.full_like(ci, OUT_SENT)
        if poisoned:
            CP.poison()
        hip.label_smooth(li, lo, ci, co, B=2, H=H, W=W, crop_h=ch, crop_w=cw, R=3)
        torch.cuda.synchronize()
        return lo, co

    a, a2, p = run(False), run(False), run(True)
    assert not CP.same_bits(a2, a, ("labels", "conf"), "two plain runs differ")
    assert not CP.same_bits(p, a, ("labels", "conf"), "the poisoned run differs")
    _same((p[0].cpu().numpy(), p[1].cpu().numpy()), SM.apply(lab, codes, cw, ch, 3))
