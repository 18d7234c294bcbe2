"""Device label stabilisation (csrc/hip/label_stable.hip) against the numpy definition
(postprocess/stable.py), and the chain / engine layers that run it first.

Every comparison is exact, on the output planes AND on the state words after the last call:
per stream [header | one word per crop pixel], header 1 once the stream has seen a frame. The
state is a view of exactly ``label_stable_state_bytes`` at the head of a larger buffer whose
sentinel tail must come back unchanged; out of place the outputs are prefilled with a sentinel
(every byte must be written) and the inputs must come back unchanged.
"""
import functools

import numpy as np
import pytest
import torch

from semantic_segmentation_server_amd.postprocess import mask_rle as MR
from semantic_segmentation_server_amd.postprocess import regions as RG
from semantic_segmentation_server_amd.postprocess import stable as SB

import stable_cases as SC

pytestmark = pytest.mark.gpu

DEV = "cuda"
TAIL, TAIL_SENT, OUT_SENT = 256, 0xA5, 0xEE


def _hip():
    from semantic_segmentation_server_amd.ops import hip_ops
    return hip_ops


class Device:
    """The kernel over a batch layout, with its carried state; mirrors ``stable_cases.Oracle``."""

    def __init__(self, N, g, counts, crop_h, crop_w):
        self.N, self.g, self.counts, self.crop_h, self.crop_w = N, g, list(counts), crop_h, crop_w
        self.nbytes = _hip().label_stable_state_bytes(len(counts), crop_h, crop_w)
        assert self.nbytes == 4 * len(counts) * (1 + crop_h * crop_w)
        self.buf = torch.zeros(self.nbytes + TAIL, dtype=torch.uint8, device=DEV)
        self.buf[self.nbytes:] = TAIL_SENT
        self.tables = _hip().label_stable_tables(counts, DEV)

    def run(self, labels, conf, inplace, counts=None):
        hip = _hip()
        counts = self.counts if counts is None else list(counts)
        tables = self.tables if counts == self.counts else hip.label_stable_tables(counts, DEV)
        B, H, W = labels.shape
        li = torch.from_numpy(labels).to(DEV)
        ci = None if conf is None else torch.from_numpy(conf).to(DEV)
        lo = li if inplace else torch.full_like(li, OUT_SENT)
        co = ci if inplace or ci is None else torch.full_like(ci, OUT_SENT)
        hip.label_stable(li, lo, ci, co, self.buf[:self.nbytes], tables, counts=counts, B=B, H=H, W=W,
                         crop_h=self.crop_h, crop_w=self.crop_w, N=self.N, g=self.g)
        torch.cuda.synchronize()
        if not inplace:
            assert np.array_equal(li.cpu().numpy(), labels)
            assert ci is None or np.array_equal(ci.cpu().numpy(), conf)
        assert (self.buf[self.nbytes:] == TAIL_SENT).all()
        return lo.cpu().numpy(), (None if co is None else co.cpu().numpy())

    def state(self):
        return self.buf[:self.nbytes].cpu().numpy().view(np.uint32)


def _same(got, want):
    assert np.array_equal(got[0], want[0])
    assert (got[1] is None) == (want[1] is None)
    assert got[1] is None or np.array_equal(got[1], want[1])


# ---- every sequence -----------------------------------------------------------------------------

@pytest.mark.parametrize("conf", [False, True])
@pytest.mark.parametrize("N", [2, 3])
def test_every_sequence_planes_as_one_batch_and_frame_by_frame(N, conf):
    if conf:
        lab, code = SC.every_sequence_conf(SC.GATE)
        g = SC.GATE
    else:
        lab, code, g = SC.every_sequence_labels(), None, 0
    T, H, W = lab.shape
    ora = SC.Oracle(N, g, [T], H, W)
    want = ora.run(lab, code)
    once = Device(N, g, [T], H, W)
    _same(once.run(lab, code, inplace=False), want)
    assert np.array_equal(once.state(), ora.state())
    step = Device(N, g, [1], H, W)
    outs = [step.run(lab[t:t + 1], None if code is None else code[t:t + 1], inplace=True) for t in range(T)]
    _same((np.concatenate([o[0] for o in outs]),
           None if code is None else np.concatenate([o[1] for o in outs])), want)
    assert np.array_equal(step.state(), once.state())
    assert (want[0] != lab).any()


# ---- geometry -----------------------------------------------------------------------------------

def _geometries():
    chunk = _hip().label_stable_chunk()
    return [(9, 13, 9, 13), (9, 13, 4, 5), (5, 7, 1, 1), (33, 33, 33, 31),
            (3, chunk + 2, 2, chunk + 1),   # a chunk boundary inside a crop row, pads on both sides
            (2, chunk + 1, 1, chunk - 1)]   # one pixel short of a full chunk


@pytest.mark.parametrize("gi", range(6))
def test_geometries_out_of_place_and_in_place(gi):
    H, W, ch, cw = _geometries()[gi]
    lab, code = SC.flicker(100 + gi, 6, H, W, flip=0.3)
    N, g, counts = 2, 100, [2]
    ora = SC.Oracle(N, g, counts, ch, cw)
    oop, inp = Device(N, g, counts, ch, cw), Device(N, g, counts, ch, cw)
    pad = np.ones((H, W), bool)
    pad[:ch, :cw] = False
    held = 0
    for k in range(3):
        l, c = lab[2 * k:2 * k + 2], code[2 * k:2 * k + 2]
        want = ora.run(l, c)
        a, b = oop.run(l, c, inplace=False), inp.run(l, c, inplace=True)
        _same(a, want), _same(b, want)
        for got, src in ((a[0], l), (a[1], c), (b[0], l), (b[1], c)):
            assert np.array_equal(got[:, pad], src[:, pad])
        held += int((want[0] != l).sum())
    assert np.array_equal(oop.state(), ora.state()) and np.array_equal(inp.state(), ora.state())
    assert held > 0 or ch * cw == 1


# ---- layouts ------------------------------------------------------------------------------------

@pytest.mark.parametrize("counts", [[3, 0, 2], [1, 1, 1, 1], [5]])
def test_batch_layouts_over_three_calls(counts):
    H, W, ch, cw = 11, 15, 10, 13
    S, B = len(counts), sum(counts)
    lab, code = SC.flicker(7 + S, S + 3 * B, H, W, flip=0.1)
    N, g = 3, 64
    ora, dev = SC.Oracle(N, g, counts, ch, cw), Device(N, g, counts, ch, cw)
    # every stream sees one frame first, so a stream without rows has a state to keep
    start = [1] * S
    ora.counts = start
    want = ora.run(lab[:S], code[:S])
    ora.counts = counts
    _same(dev.run(lab[:S], code[:S], inplace=True, counts=start), want)
    after_start = dev.state().reshape(S, -1).copy()
    assert (after_start[:, 0] == 1).all()
    for k in range(3):
        sl = slice(S + k * B, S + (k + 1) * B)
        want = ora.run(lab[sl], code[sl])
        _same(dev.run(lab[sl], code[sl], inplace=bool(k % 2)), want)
        assert np.array_equal(dev.state(), ora.state()), k
    now = dev.state().reshape(S, -1)
    for s, c in enumerate(counts):
        assert np.array_equal(now[s], after_start[s]) == (c == 0)


def test_a_stream_that_never_had_a_row_stays_all_zero():
    counts, ch, cw = [2, 0], 5, 6
    lab, _ = SC.flicker(3, 2, 6, 7)
    ora, dev = SC.Oracle(2, 0, counts, ch, cw), Device(2, 0, counts, ch, cw)
    _same(dev.run(lab, None, inplace=False), ora.run(lab, None))
    st = dev.state().reshape(2, -1)
    assert not st[1].any() and st[0, 0] == 1 and np.array_equal(dev.state(), ora.state())


# ---- without confidence planes, N limits --------------------------------------------------------

def test_without_conf_planes_h_stays_zero_and_a_gate_is_refused():
    H, W, ch, cw = 9, 13, 8, 11
    lab, _ = SC.flicker(21, 6, H, W, flip=0.2)
    ora, dev = SC.Oracle(2, 0, [3], ch, cw), Device(2, 0, [3], ch, cw)
    for k in range(2):
        got = dev.run(lab[3 * k:3 * k + 3], None, inplace=bool(k))
        _same(got, ora.run(lab[3 * k:3 * k + 3], None))
    assert np.array_equal(dev.state(), ora.state())
    assert not (dev.state()[1:] >> 24).any()
    gated = Device(2, 5, [3], ch, cw)
    with pytest.raises(ValueError, match="g 5 > 0 needs the conf planes"):
        gated.run(lab[:3], None, inplace=True)
    assert not gated.state().any()


def test_n_2_and_n_255_on_a_3x3_plane():
    # N = 2: the second sight of a new label switches
    lab = np.zeros((4, 3, 3), np.uint8)
    lab[1:, 0, 0], lab[2, 1, 1], lab[3, 2, 2] = 9, 4, 4
    ora, dev = SC.Oracle(2, 0, [4], 3, 3), Device(2, 0, [4], 3, 3)
    want = ora.run(lab, None)
    _same(dev.run(lab, None, inplace=False), want)
    assert want[0][:, 0, 0].tolist() == [0, 0, 9, 9] and not want[0][:, 1:, 1:].any()
    assert np.array_equal(dev.state(), ora.state())
    # N = 255: one frame starts the stream, then one call of B = 255; pixel j sees the new label
    # from row j on -- pixel 0 for 255 frames (it switches in the last one), the others fewer
    first = np.full((1, 3, 3), 3, np.uint8)
    seq = np.full((255, 9), 3, np.uint8)
    for j in range(9):
        seq[j:, j] = 200
    seq = seq.reshape(255, 3, 3)
    ora, dev = SC.Oracle(255, 0, [255], 3, 3), Device(255, 0, [255], 3, 3)
    ora.counts = [1]
    _same(dev.run(first, None, inplace=True, counts=[1]), ora.run(first, None))
    ora.counts = [255]
    want = ora.run(seq, None)
    _same(dev.run(seq, None, inplace=False), want)
    flat = want[0].reshape(255, 9)
    assert (flat[:254] == 3).all() and flat[254].tolist() == [200] + [3] * 8
    assert np.array_equal(dev.state(), ora.state())
    s, c, n, h = SB.unpack(dev.state()[1:])
    assert (s[0], c[0], n[0]) == (200, 200, 0) and n[1:].tolist() == list(range(254, 246, -1))


# ---- wrapper refusals ---------------------------------------------------------------------------

def test_wrapper_refusals_name_the_argument():
    hip = _hip()
    B, H, W, ch, cw, counts = 2, 6, 7, 5, 6, [1, 1]
    lab = torch.zeros((B, H, W), dtype=torch.uint8, device=DEV)
    cf = torch.zeros_like(lab)
    state = torch.zeros(hip.label_stable_state_bytes(2, ch, cw), dtype=torch.uint8, device=DEV)
    tables = hip.label_stable_tables(counts, DEV)
    kw = dict(counts=counts, B=B, H=H, W=W, crop_h=ch, crop_w=cw, N=3, g=0)

    def bad(match, exc=ValueError, args=None, **over):
        a = dict(labels_in=lab, labels_out=lab, conf_in=cf, conf_out=cf, state=state, tables=tables)
        a.update(args or {})
        with pytest.raises(exc, match=match):
            hip.label_stable(a["labels_in"], a["labels_out"], a["conf_in"], a["conf_out"], a["state"],
                             a["tables"], **{**kw, **over})

    bad("labels_in", TypeError, args=dict(labels_in=lab.to(torch.int32)))
    bad("conf_out", TypeError, args=dict(conf_out=cf.to(torch.int16)))
    bad("labels_out: shape", args=dict(labels_out=torch.zeros((B, H, W + 1), dtype=torch.uint8, device=DEV)))
    bad("state: ", args=dict(state=torch.zeros(state.numel() + 4, dtype=torch.uint8, device=DEV)))
    bad("state: ", args=dict(state=state[:-4]))
    bad("counts", counts=[1, 2])
    bad("counts", counts=[1, 1], B=3)
    bad("tables: 3 words", args=dict(tables=tables[:3]))
    bad("state: ", counts=[2])  # one stream: another state size
    bad("N 1 outside", N=1)
    bad("N 256 outside", N=256)
    bad("g 256 outside", g=256)
    bad("crop", crop_w=W + 1)
    bad("crop", crop_h=0)
    bad("both given or both None", args=dict(conf_out=None))
    bad("needs the conf planes", args=dict(conf_in=None, conf_out=None), g=1)
    bad("overlap", args=dict(conf_in=lab, conf_out=lab))
    torch.cuda.synchronize()
    assert not state.any()


# ---- the chain, eager and captured ---------------------------------------------------------------

CH_H = CH_W = 33
CROP_H, CROP_W = 33, 31
CLS, KS, CAP = tuple(range(1, 8)), 16, 1100


def _chain_maps(T):
    lab, code = SC.flicker(41, T, CH_H, CH_W, flip=0.1, block=5)
    return (lab % 8).astype(np.uint8), code


def _chain(conf):
    from semantic_segmentation_server_amd.postprocess.device import DevicePostprocess
    return DevicePostprocess(torch.device(DEV), CH_H, CH_W, np.zeros((256, 3), np.int32), K=8, bins=8,
                             mask_cap=CAP, region_cap=KS, region_classes=RG.class_mask(CLS),
                             region_min_pixels=3, region_conf=conf, stable_frames=3,
                             stable_gate=90 if conf else 0, stable_streams=1)


def _chain_want(lab, code, conf):
    st = SB.Stabilizers(3, 90 if conf else 0)
    out = []
    for t in range(len(lab)):
        l, c = st.step(lab[t:t + 1], code[t:t + 1] if conf else None, CROP_W, CROP_H, [0])
        rw = 7 if conf else 6
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


@pytest.mark.parametrize("conf", [False, True])
def test_chain_eager_and_captured_equal_the_host_chain(conf):
    lab, code = _chain_maps(5)
    want = _chain_want(lab, code, conf)
    assert any((w[0] != lab[t]).any() for t, w in enumerate(want))
    dp = _chain(conf)
    assert dp.track_counts(1) == [1]
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
    dp.reset_tracks()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
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
    dp.reset_tracks()
    load(4)  # after a reset the next step is a first frame: the raw map passes
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(lab_t[0].cpu().numpy(), lab[4])
    assert not conf or np.array_equal(cf_t[0].cpu().numpy(), code[4])


def test_flag_off_makes_no_buffer_and_no_launch():
    from semantic_segmentation_server_amd.postprocess.device import DevicePostprocess
    dp = DevicePostprocess(torch.device(DEV), CH_H, CH_W, np.zeros((256, 3), np.int32), K=8, bins=8,
                           mask_cap=CAP)
    lab, _ = _chain_maps(2)
    lab_t = torch.from_numpy(lab[:1].copy()).to(DEV)
    dp.run(lab_t, CROP_W, CROP_H, 4.0)
    dp.run(lab_t.copy_(torch.from_numpy(lab[1:2])), CROP_W, CROP_H, 4.0)
    torch.cuda.synchronize()
    assert dp.stable_frames == 0 and not dp._stable_state and not dp._stable_tables
    assert np.array_equal(lab_t.cpu().numpy(), lab[1:2])


# ---- engine with graphs -------------------------------------------------------------------------

def _cfg(**kw):
    from semantic_segmentation_server_amd import config as C
    base = dict(input_size=129, batch=1, streams=1, backend="hip", graph=True, min_area_ratio=0.0005,
                serve_masks=True, serve_regions=True, track_regions=True, region_min_area_ratio=0.001)
    base.update(kw)
    return C.Config(**base)


@functools.lru_cache(maxsize=None)
def _frames():
    from semantic_segmentation_server_amd.runtime.sources import SyntheticSource
    src = SyntheticSource(160, 120, pool=2, seed=11)
    return [src.read_batch(1)[0].copy() for _ in range(2)]


def _engine_steps(eng, seq):
    out = []
    for k, f in enumerate(seq):
        eng.step(f, [k], [0.0], 0)
        out.append((eng.masks[0].copy(), eng.regions[0].copy()))
    return out


def test_engine_with_host_post_processing_stabilises_on_the_host():
    from semantic_segmentation_server_amd.runtime.engine import Engine
    A, B = _frames()
    eng = Engine(_cfg(stable_labels=3, contour_mode="exact", track_regions=False), torch.device(DEV))
    eng.set_camera(160, 120)
    raw = [eng._infer_eager(torch.from_numpy(f).to(DEV)).cpu().numpy()[0] for f in (A, B)]
    cw, ch = eng.crop_w, eng.crop_h
    got = _engine_steps(eng, [A, B, B, B])
    st = SB.StreamStabilizer(3)
    for k, i in enumerate((0, 1, 1, 1)):
        lab, _ = st.step(raw[i], None, cw, ch)
        assert np.array_equal(MR.decode(got[k][0]), lab[:ch, :cw]), k
        want = RG.encode(lab, cw, ch, eng.region_mask, eng.region_min_pixels, eng.region_cap)
        u = RG.used_words(want, eng.region_cap)
        assert np.array_equal(got[k][1][:u], want[:u]), k
    assert np.array_equal(MR.decode(got[2][0]), raw[0][:ch, :cw])
    assert np.array_equal(MR.decode(got[3][0]), raw[1][:ch, :cw])
    # the label maps of the step are the stabilised ones, on the device too
    assert np.array_equal(eng._static["labels"][0].cpu().numpy(), lab)  # pad rows: the raw map's


def test_engine_with_graphs_serves_the_stabilised_maps():
    from semantic_segmentation_server_amd.postprocess import tracks as TK
    from semantic_segmentation_server_amd.runtime.engine import Engine
    A, B = _frames()
    # one engine for both sequences (reset_tracks in between); its model's raw label maps come
    # from the eager path, which the stabilisation (a post-processing launch) does not touch
    eng = Engine(_cfg(stable_labels=3), torch.device(DEV))
    assert eng.stable_frames == 3 and eng.stable_streams == 1
    eng.set_camera(160, 120)
    raw = [eng._infer_eager(torch.from_numpy(f).to(DEV)).cpu().numpy()[0] for f in (A, B)]
    cw, ch = eng.crop_w, eng.crop_h
    assert (raw[0][:ch, :cw] != raw[1][:ch, :cw]).any()
    for order in ((0, 1, 0, 1), (0, 1, 1, 1)):
        eng.reset_tracks()
        got = _engine_steps(eng, [(A, B)[i] for i in order])
        st, trk = SB.StreamStabilizer(3), TK.StreamTracker(eng.track_q)
        for k, i in enumerate(order):
            lab, _ = st.step(raw[i], None, cw, ch)
            want_mask = MR.encode(lab, cw, ch, eng.mask_cap)
            want_reg = RG.encode(lab, cw, ch, eng.region_mask, eng.region_min_pixels, eng.region_cap,
                                 out=np.zeros(4 + 8 * eng.region_cap, np.uint32), tracker=trk)
            u = MR.used_words(want_mask)
            assert np.array_equal(got[k][0][:u], want_mask[:u]), (order, k)
            u = RG.used_words(want_reg, eng.region_cap, tracks=True)
            assert np.array_equal(got[k][1][:u], want_reg[:u]), (order, k)
        masks = [MR.decode(m) for m, _ in got]
        assert np.array_equal(masks[0], raw[0][:ch, :cw])
        if order == (0, 1, 0, 1):
            assert all(np.array_equal(m, masks[0]) for m in masks[1:])
            ages = [RG.decode(r, tracks=True)["age"] for _, r in got]
            assert all((a == k + 1).all() for k, a in enumerate(ages))  # no track ever ends
        else:
            assert np.array_equal(masks[1], masks[0]) and np.array_equal(masks[2], masks[0])
            assert np.array_equal(masks[3], raw[1][:ch, :cw]) and not np.array_equal(masks[3], masks[2])
        # the step hands out the stabilised label maps themselves
        assert np.array_equal(eng._static["labels"][0].cpu().numpy()[:ch, :cw], masks[3])
