"""Per-pixel confidence on the device (--serve_confidence): the two-plane upsample kernel
(csrc/hip/model_ops.hip ``upsample_argmax_conf``) against float64, the class-region kernels
with the seventh word ``sum_conf`` against the numpy definition (postprocess/regions.py), and
the plan / engine / pipeline layers that carry the confidence plane.

Bounds of the kernel test (they come from the arithmetic, not from the kernel's output):
with p64 the float64 softmax maximum of the float64 bilinear interpolant of the same bf16
logits, ``|conf - 255 p64| <= 0.5 + 0.01`` at EVERY pixel. 0.5 is the rounding to a code. The
0.01: for |logit| <= 32 the three fp32 lerps err by < 8e-6, which moves p by < 4e-6; a few-ulp
exp, the K-term sum, the reciprocal and the shared rounding of the subtrahend add < 5e-6:
about 2.6e-3 codes in all, a margin of about 4 x. Labels equal the float64 argmax wherever the
float64 top-two margin exceeds 1e-4 (over 10 x the interpolation bound); the inputs must leave
at most 0.2 % of the map below that margin.
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from semantic_segmentation_server_amd.postprocess import regions as RG
from upsample_ref import GUARD, guarded as _guarded, ref64 as _ref64

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENT = 0x5A5A5A5A
WS_SENT = 0xA5
WS_TAIL = 256


def _hip():
    from semantic_segmentation_server_amd.ops import hip_ops
    return hip_ops


# ---- the kernel against float64 ---------------------------------------------------------------

CASES = [(2, 9, 9, 65, 65, 21),      # KC = 21
         (2, 9, 9, 65, 65, 19),      # KC = 19
         (2, 33, 33, 257, 257, 30),  # runtime K, KP = 32
         (2, 5, 5, 40, 40, 40),      # K > 32: the direct kernel
         (3, 9, 13, 65, 97, 21)]     # non-square; the last lanes of a wave are past the map


def _logits(B, h, w, K, field):
    """As tests/test_hip_kernels.py::test_upsample_argmax builds them, with the padding
    channels K .. ldk at +100: a padded class in the maximum or the sum fails the test."""
    g = torch.Generator().manual_seed(7)
    ldk = (K + 7) // 8 * 8
    if field == "noise":
        logits = torch.randn(B, h, w, ldk, generator=g).to(torch.bfloat16)
    else:
        coarse = torch.randn(B, ldk, 4, 4, generator=g) * 4
        logits = F.interpolate(coarse, size=(h, w), mode="bilinear", align_corners=True) \
            .permute(0, 2, 3, 1).contiguous().to(torch.bfloat16)
    logits[..., K:] = 100.0
    return logits, ldk


def _assert_conf(conf, labels, c64, a64, margin, input_condition=True):
    err = (conf.double() - c64).abs().max().item()
    decided = margin > 1e-4
    undecided = 1.0 - decided.double().mean().item()
    wrong = int((labels.long() != a64)[decided].sum())
    print(f"max |conf - 255 p64| = {err:.6f}, undecided {100 * undecided:.4f} %, wrong labels {wrong}")
    assert err <= 0.5 + 0.01, err
    assert not input_condition or undecided <= 0.002, undecided  # a condition on the test's inputs
    assert wrong == 0, wrong


@pytest.mark.parametrize("field", ["noise", "smooth"])
@pytest.mark.parametrize("B,h,w,H,W,K", CASES)
def test_kernel_against_float64(B, h, w, H, W, K, field):
    logits, ldk = _logits(B, h, w, K, field)
    assert logits[..., :K].float().abs().max() < 32
    c64, a64, margin = _ref64(logits, K, H, W)
    raw_l, labels = _guarded(B, H, W)
    raw_c, conf = _guarded(B, H, W)
    _hip().upsample_argmax_conf(logits.to(DEV), labels, conf, B=B, h=h, w=w, K=K, ldk=ldk, H=H, W=W)
    torch.cuda.synchronize()
    for raw in (raw_l, raw_c):
        r = raw.cpu()
        assert (r[0] == GUARD).all() and (r[-1] == GUARD).all()
    _assert_conf(conf.cpu(), labels.cpu(), c64, a64, margin)
    assert int(conf.min()) >= int(np.floor(255.0 / K + 0.5 - 0.01))  # p >= 1 / K


def test_the_kernel_computes_the_definition():
    """Against ops/reference_ops.upsample_confidence (fp32): codes within one step, and equal
    wherever 255 p64 is not within 0.02 of a rounding boundary."""
    from semantic_segmentation_server_amd.ops import reference_ops as R
    B, h, w, H, W, K = CASES[0]
    logits, ldk = _logits(B, h, w, K, "smooth")
    lab_ref, conf_ref = R.upsample_confidence(logits[..., :K].permute(0, 3, 1, 2).float(), H, W)
    c64, _, margin = _ref64(logits, K, H, W)
    labels = torch.empty((B, H, W), dtype=torch.uint8, device=DEV)
    conf = torch.empty_like(labels)
    _hip().upsample_argmax_conf(logits.to(DEV), labels, conf, B=B, h=h, w=w, K=K, ldk=ldk, H=H, W=W)
    d = (conf.cpu().int() - conf_ref.int()).abs()
    clear = ((c64 + 0.5) - torch.floor(c64 + 0.5) - 0.5).abs() < 0.48  # away from x.5
    assert d.max() <= 1 and int(d[clear].sum()) == 0
    assert torch.equal(labels.cpu()[margin > 1e-4], lab_ref[margin > 1e-4])


def test_wrapper_rejects_bad_arguments_without_launching():
    B, h, w, H, W, K, ldk = 1, 3, 3, 9, 9, 5, 8
    logits = torch.zeros((B, h, w, ldk), dtype=torch.bfloat16, device=DEV)
    raw_l, labels = _guarded(B, H, W)
    raw_c, conf = _guarded(B, H, W)

    def go(logits=logits, labels=labels, conf=conf, **kw):
        a = dict(B=B, h=h, w=w, K=K, ldk=ldk, H=H, W=W)
        a.update(kw)
        _hip().upsample_argmax_conf(logits, labels, conf, **a)

    with pytest.raises(TypeError):
        go(logits=logits.float())
    with pytest.raises(TypeError):
        go(conf=conf.to(torch.int8))
    with pytest.raises(TypeError):
        go(labels=labels.to(torch.int32))
    with pytest.raises(ValueError):
        go(conf=torch.zeros((B, H, W), dtype=torch.uint8))  # on the host
    with pytest.raises(ValueError):
        go(labels=torch.zeros((B, H, W), dtype=torch.uint8))
    with pytest.raises(ValueError):
        go(conf=torch.zeros((B, H, 2 * W), dtype=torch.uint8, device=DEV)[:, :, ::2])  # strided
    with pytest.raises(ValueError):
        go(conf=torch.zeros((B, H, W + 1), dtype=torch.uint8, device=DEV))  # wrong shape
    with pytest.raises(ValueError):
        go(labels=torch.zeros((B, H * W), dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError):
        go(conf=labels)  # one plane for both
    with pytest.raises(ValueError):
        go(h=4)  # logits too small
    with pytest.raises(ValueError):
        go(K=9)  # K > ldk
    with pytest.raises(ValueError):
        go(K=0)
    with pytest.raises(ValueError):
        go(logits=torch.zeros((B, h, w, 264), dtype=torch.bfloat16, device=DEV), K=257, ldk=264)
    torch.cuda.synchronize()
    assert (raw_l.cpu() == GUARD).all() and (raw_c.cpu() == GUARD).all()


# ---- regions with sum_conf ----------------------------------------------------------------------

def _want(labels, confs, crop_h, crop_w, classes, min_pixels, K):
    rw = 6 if confs is None else 7
    return np.stack([RG.encode(l, crop_w, crop_h, classes, min_pixels, K,
                               out=np.full(4 + rw * K, SENT, np.uint32),
                               conf=None if confs is None else confs[b]) for b, l in enumerate(labels)])


def _check(labels, confs, crop_h, crop_w, classes, min_pixels=2, K=16):
    """Launch with the confidence planes: every word of the [B, 4 + 7 K] rows (header,
    records, untouched sentinel words) equals the definition's, and the workspace tail is
    untouched. Without the planes the same call gives today's 6-word rows."""
    hip = _hip()
    labels = np.ascontiguousarray(labels, np.uint8)
    confs = np.ascontiguousarray(confs, np.uint8)
    B, H, W = labels.shape
    lab, cf = torch.from_numpy(labels).to(DEV), torch.from_numpy(confs).to(DEV)
    tabs = None
    for with_conf in (True, False):
        rw = 7 if with_conf else 6
        nb = hip.class_regions_workspace_bytes(B, crop_h, crop_w, with_conf)
        out = torch.full((B, 4 + rw * K), SENT, dtype=torch.int32, device=DEV)
        ws = torch.full((nb + WS_TAIL,), WS_SENT, dtype=torch.uint8, device=DEV)
        hip.class_regions(lab, out, ws, B=B, H=H, W=W, crop_h=crop_h, crop_w=crop_w, classes=classes,
                          min_pixels=min_pixels, K=K, **({"conf": cf} if with_conf else {}))
        torch.cuda.synchronize()
        got = out.cpu().numpy().view(np.uint32)
        want = _want(labels, confs if with_conf else None, crop_h, crop_w, classes, min_pixels, K)
        for b in range(B):
            assert np.array_equal(got[b], want[b]), (with_conf, b, np.flatnonzero(got[b] != want[b])[:8])
        assert (ws[nb:].cpu().numpy() == WS_SENT).all()
        if with_conf:
            tabs = [RG.decode(g, conf=True) for g in got]
    return tabs


def _blobs(rng, H, W, classes=6, cell=8, noise=0.03):
    coarse = rng.integers(0, classes, (H // cell + 1, W // cell + 1)).astype(np.uint8)
    lab = np.repeat(np.repeat(coarse, cell, 0), cell, 1)[:H, :W].copy()
    sp = rng.random((H, W)) < noise
    lab[sp] = rng.integers(0, classes, int(sp.sum()))
    return lab


def test_ragged_crop_across_tile_corners():
    """A 45 x 70 crop of a 64 x 96 map (no multiple of the 32-pixel tile; blobs of 8 x 8 cells
    span tile edges and corners), three frames, the last with every code 255."""
    H, W, ch, cw = 64, 96, 45, 70
    rng = np.random.default_rng(2)
    labels = np.stack([_blobs(rng, H, W) for _ in range(3)])
    confs = rng.integers(0, 256, (3, H, W)).astype(np.uint8)
    confs[2] = 255
    tabs = _check(labels, confs, ch, cw, [1, 2, 3, 4, 5], 4, 32)
    assert all(len(t) > 4 for t in tabs)
    assert np.array_equal(tabs[2]["sum_conf"], 255 * tabs[2]["pixels"])


def test_one_region_covers_the_frame():
    """Every tile adds to one slot (the bucketed atomics); all codes 255 is the largest sum."""
    H, W, ch, cw = 101, 101, 97, 73
    rng = np.random.default_rng(3)
    confs = rng.integers(0, 256, (2, H, W)).astype(np.uint8)
    confs[1] = 255
    tabs = _check(np.full((2, H, W), 5, np.uint8), confs, ch, cw, [5])
    assert [len(t) for t in tabs] == [1, 1]
    assert tabs[0][0]["sum_conf"] == int(confs[0, :ch, :cw].astype(np.int64).sum())
    assert tabs[1][0]["sum_conf"] == 255 * ch * cw


def test_serpentine_and_checkerboard():
    H, W, ch, cw = 101, 101, 73, 97
    rng = np.random.default_rng(4)
    snake = np.zeros((H, W), np.uint8)
    snake[0:ch:2, :cw] = 3
    for k, y in enumerate(range(1, ch - 1, 2)):
        snake[y, cw - 1 if k % 2 == 0 else 0] = 3
    snake[ch:, :] = 3  # outside the crop: ignored
    snake[:, cw:] = 3
    snake_t = np.zeros((H, W), np.uint8)
    snake_t[:ch, 0:cw:2] = 3
    for k, x in enumerate(range(1, cw - 1, 2)):
        snake_t[ch - 1 if k % 2 == 0 else 0, x] = 3
    y, x = np.mgrid[:H, :W]
    board = (1 + ((x + y) & 1)).astype(np.uint8)
    confs = rng.integers(0, 256, (3, H, W)).astype(np.uint8)
    tabs = _check(np.stack([snake, snake_t, board]), confs, ch, cw, [1, 2, 3])
    assert [len(t) for t in tabs] == [1, 1, 2]
    on = snake[:ch, :cw] == 3
    assert tabs[0][0]["sum_conf"] == int(confs[0, :ch, :cw][on].astype(np.int64).sum())


def test_cut_off_and_a_frame_without_regions():
    """More passing regions than K: the true count and K seven-word records; a frame of
    unserved classes writes its header alone."""
    H, W, ch, cw = 64, 96, 45, 70
    rng = np.random.default_rng(5)
    labels = np.stack([_blobs(rng, H, W), np.zeros((H, W), np.uint8), _blobs(rng, H, W, noise=0.0)])
    confs = rng.integers(0, 256, (3, H, W)).astype(np.uint8)
    tabs = _check(labels, confs, ch, cw, [1, 2, 3, 4, 5], 3, 4)
    want = _want(labels, confs, ch, cw, [1, 2, 3, 4, 5], 3, 4)
    assert want[0, 0] > 4 and want[2, 0] > 4 and want[1, 0] == 0
    assert [len(t) for t in tabs] == [4, 0, 4]
    assert RG.used_words(want[0], conf=True) == 4 + 7 * 4 and RG.used_words(want[1], conf=True) == 4


def test_regions_wrapper_rejects_a_bad_conf_plane():
    hip = _hip()
    lab = torch.zeros((1, 9, 7), dtype=torch.uint8, device=DEV)
    out = torch.full((1, 4 + 7 * 8), SENT, dtype=torch.int32, device=DEV)
    ws = torch.full((hip.class_regions_workspace_bytes(1, 9, 7, True),), WS_SENT, dtype=torch.uint8, device=DEV)
    ok = dict(B=1, H=9, W=7, crop_h=9, crop_w=7, classes=[1], min_pixels=1, K=8)
    with pytest.raises(TypeError):
        hip.class_regions(lab, out, ws, conf=lab.to(torch.int32), **ok)
    with pytest.raises(ValueError):
        hip.class_regions(lab, out, ws, conf=torch.zeros((1, 9, 8), dtype=torch.uint8, device=DEV), **ok)
    with pytest.raises(ValueError):
        hip.class_regions(lab, out, ws, conf=torch.zeros((1, 9, 7), dtype=torch.uint8), **ok)
    with pytest.raises(ValueError):  # rows of 6 words with a conf plane
        hip.class_regions(lab, out[:, :4 + 6 * 8].contiguous(), ws, conf=lab, **ok)
    with pytest.raises(ValueError):  # the workspace of the form without confidence
        hip.class_regions(lab, out, ws[:hip.class_regions_workspace_bytes(1, 9, 7)], conf=lab, **ok)
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == SENT).all() and (ws.cpu().numpy() == WS_SENT).all()


# ---- capture -------------------------------------------------------------------------------------

def test_kernel_and_regions_captured_in_a_graph_and_replayed_on_new_inputs():
    hip = _hip()
    B, h, w, H, W, K = 2, 9, 9, 65, 65, 21
    cls, mp, cap = RG.default_classes(K), 3, 16
    inputs = [_logits(B, h, w, K, f)[0] for f in ("smooth", "noise")]
    ldk = inputs[0].shape[-1]
    logits = torch.zeros((B, h, w, ldk), dtype=torch.bfloat16, device=DEV)
    labels = torch.zeros((B, H, W), dtype=torch.uint8, device=DEV)
    conf = torch.zeros_like(labels)
    nb = hip.class_regions_workspace_bytes(B, H, W, True)
    out = torch.full((B, 4 + 7 * cap), SENT, dtype=torch.int32, device=DEV)
    ws = torch.full((nb + WS_TAIL,), WS_SENT, dtype=torch.uint8, device=DEV)

    def run():
        hip.upsample_argmax_conf(logits, labels, conf, B=B, h=h, w=w, K=K, ldk=ldk, H=H, W=W)
        hip.class_regions(labels, out, ws, B=B, H=H, W=W, crop_h=H, crop_w=W, classes=cls,
                          min_pixels=mp, K=cap, conf=conf)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        run()
    for x in inputs:
        logits.copy_(x)
        out.fill_(SENT)
        g.replay()
        torch.cuda.synchronize()
        lab, cf = labels.cpu(), conf.cpu()
        _assert_conf(cf, lab, *_ref64(x, K, H, W))
        want = _want(lab.numpy(), cf.numpy(), H, W, cls, mp, cap)
        assert np.array_equal(out.cpu().numpy().view(np.uint32), want)
    assert (ws[nb:].cpu().numpy() == WS_SENT).all()


# ---- plan, engine, pipeline ----------------------------------------------------------------------

def _cfg(**kw):
    from semantic_segmentation_server_amd import config as C
    base = dict(input_size=129, batch=2, backend="hip", graph=False, min_area_ratio=0.0005)
    base.update(kw)
    return C.Config(**base)


@functools.lru_cache(maxsize=None)
def _engine(graph, confidence):
    from semantic_segmentation_server_amd.runtime.engine import Engine
    return Engine(_cfg(graph=graph, serve_regions=True, serve_confidence=confidence), torch.device(DEV))


def _want_engine(eng, labels, conf=None):
    return np.stack([RG.encode(l, eng.crop_w, eng.crop_h, eng.region_mask, eng.region_min_pixels,
                               eng.region_cap, conf=None if conf is None else conf[b])
                     for b, l in enumerate(labels)])


@pytest.mark.parametrize("graph", [False, True])
def test_engine_step_carries_the_confidence_of_its_own_logits(graph):
    from semantic_segmentation_server_amd.runtime.sources import SyntheticSource
    eng = _engine(graph, True)
    src = SyntheticSource(200, 150, pool=4, seed=7)
    for k in range(2):
        f, _, _ = src.read_batch(2)
        ids, ts = [2 * k, 2 * k + 1], [1.0, 2.0]
        recs = eng.step(f, ids, ts, [0, 1])
        got = eng.regions.copy()
        bufs = eng._hip_model.buffers(2, 150, 200)
        assert eng.conf_plane is not None and eng.conf_plane.data_ptr() == bufs["conf"].data_ptr()
        labels, conf = bufs["labels"].cpu(), bufs["conf"].cpu()
        K = eng.cfg.num_classes
        # (a) at every pixel; the model's own near-ties are not an input this test chooses
        _assert_conf(conf, labels, *_ref64(bufs["logits"].cpu(), K, eng.H, eng.W), input_condition=False)
        assert got.shape == (2, 4 + 7 * 64) and got.dtype == np.uint32
        want = _want_engine(eng, labels.numpy(), conf.numpy())
        for b in range(2):
            used = RG.used_words(want[b], conf=True)
            assert used > 4 and np.array_equal(got[b, :used], want[b, :used]), b
        # the records of the step are the records of those labels
        rec = eng._device_post(bufs["labels"], conf=bufs["conf"])
        again = eng._hip_post.fetch(rec, ids, ts, [0, 1], eng.W, eng.H)
        assert len(recs) > 0 and recs.tobytes() == again.tobytes()


def test_flag_off_keeps_the_plan_and_the_six_word_rows():
    """The structural condition: without the flag the plan has the steps and buffers it had
    (the last step is the "upsample" choice over the four label kernels, no "conf" buffer);
    with it, the same steps but the last, and one more buffer."""
    from semantic_segmentation_server_amd.models.plan import Choice
    from semantic_segmentation_server_amd.runtime.sources import SyntheticSource
    on, off = _engine(False, True), _engine(False, False)
    f, _, _ = SyntheticSource(200, 150, pool=2, seed=7).read_batch(2)
    for eng in (on, off):
        eng.step(f, [0, 1], [1.0, 2.0], [0, 1])
    ops_on, bufs_on = on._hip_model._plan(2, 150, 200)
    ops_off, bufs_off = off._hip_model._plan(2, 150, 200)
    assert set(bufs_on) == set(bufs_off) | {"conf"} and "conf" not in bufs_off
    assert {n: tuple(t.shape) for n, t in bufs_off.items()} == \
        {n: tuple(t.shape) for n, t in bufs_on.items() if n != "conf"}
    last = ops_off[-1]
    assert isinstance(last, Choice) and last.name == "upsample"
    assert [n for n, _ in last.variants] == ["rows", "lane", "union", "cand"]
    assert not isinstance(ops_on[-1], Choice) and len(ops_on) == len(ops_off)
    assert [op.name for op in ops_on[:-1] if isinstance(op, Choice)] == \
        [op.name for op in ops_off[:-1] if isinstance(op, Choice)]
    assert "upsample" not in on._hip_model.choices and "upsample" in off._hip_model.choices
    assert off.conf_plane is None and off.region_words == 6 and not off._hip_post.region_conf
    assert off.regions.shape == (2, 4 + 6 * 64)
    labels = bufs_off["labels"].cpu().numpy()
    want = _want_engine(off, labels)
    for b in range(2):
        used = RG.used_words(want[b])
        assert np.array_equal(off.regions[b, :used], want[b, :used])
    with pytest.raises(ValueError):
        off._hip_model.segment(torch.from_numpy(f).to(DEV), off.lut_x, off.lut_y,
                               conf_out=torch.zeros((2, 129, 129), dtype=torch.uint8, device=DEV))


FORMS = {"slot": dict(env={"SSA_SLOT_PARALLEL": "1", "SSA_MODEL_PARTS": "1"}, batch=2, lag=2, cfg={}),
         "split": dict(env={"SSA_SLOT_PARALLEL": "0", "SSA_MODEL_PARTS": "1"}, batch=2, lag=1, cfg={}),
         "parts": dict(env={"SSA_SLOT_PARALLEL": "0", "SSA_MODEL_PARTS": "2"}, batch=4, lag=1, cfg={}),
         "torch": dict(env={}, batch=2, lag=1, cfg=dict(backend="torch"))}


@pytest.mark.parametrize("form", list(FORMS))
def test_every_graph_form_carries_its_own_confidence_plane(monkeypatch, form):
    """The pipeline's captured step forms (runtime/capture.py): slot-parallel plan copies at
    lag 2, the split model / post-processing graphs, two sub-batch parts, and the torch backend's
    split step. Every step object owns its confidence plane, and the hub's latest regions are
    those of the last step's own labels and plane."""
    from semantic_segmentation_server_amd.parallel import dist as D
    from semantic_segmentation_server_amd.parallel.dp import DataParallelPipeline
    from semantic_segmentation_server_amd.runtime import capture
    from semantic_segmentation_server_amd.runtime.engine import Engine
    from semantic_segmentation_server_amd.runtime.results import ResultHub
    from semantic_segmentation_server_amd.runtime.sources import SyntheticSource
    f = FORMS[form]
    for k, v in f["env"].items():
        monkeypatch.setenv(k, v)
    B, lag = f["batch"], f["lag"]
    n = 2 * (lag + 1) + 1
    src = SyntheticSource(160, 120, pool=B * n, seed=11)
    batches = [torch.from_numpy(src.read_batch(B)[0].copy()) for _ in range(n)]
    eng = Engine(_cfg(graph=True, serve_regions=True, serve_confidence=True, batch=B, **f["cfg"]),
                 torch.device(DEV))
    hub = ResultHub(B, maxlen=100000)
    pipe = DataParallelPipeline(D.init(), eng, 160, 120, B, "local", hub, B, lag=lag, auto_lag=False)
    assert pipe.lag == lag and pipe.nslots == lag + 1
    pipe.prefetch(batches[0].pin_memory())
    for k in range(n):
        pipe.step(frame_ids=[100 + B * k + i for i in range(B)], ts=[1.0 + k] * B, streams=list(range(B)),
                  next_frames=batches[k + 1].pin_memory() if k + 1 < n else None)
    pipe.flush()
    torch.cuda.synchronize()
    steps = list(eng._bound_graphs.values())
    kind = {"slot": capture.SlotStep, "split": capture.SplitStep, "parts": capture.PartsStep,
            "torch": capture.SplitStep}[form]
    assert len(steps) == lag + 1 and all(type(s) is kind for s in steps)
    assert len({s.conf.data_ptr() for s in steps}) == lag + 1 == len({s.labels.data_ptr() for s in steps})
    labels, _ = eng.run_device(pipe.staging[pipe.slot])  # the last step's slot still holds its frames
    torch.cuda.synchronize()
    conf = eng.conf_plane
    assert conf is not None and conf.shape == labels.shape and conf.dtype == torch.uint8
    want = _want_engine(eng, labels.cpu().numpy(), conf.cpu().numpy())
    for s in range(B):
        r = hub.regions(s)
        assert r is not None and r.conf and r.frame_id == 100 + B * (n - 1) + s
        assert len(r.words) == RG.used_words(want[s], conf=True) > 4
        assert np.array_equal(r.words, want[s][:len(r.words)])
        tab = RG.decode(r.words, conf=True)
        px = tab["pixels"].astype(np.int64)
        assert (tab["sum_conf"] <= 255 * px).all() and (tab["sum_conf"] >= 12 * px).all()  # p >= 1 / 21
