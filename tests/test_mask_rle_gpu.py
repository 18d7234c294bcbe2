"""Device run-length encoder of the label masks (csrc/hip/mask_rle.hip) against the numpy
definition (postprocess/mask_rle.py), and the engine / pipeline layers that carry its output.

Every kernel case compares the device words with ``mask_rle.encode`` exactly, on the header
and on the stored runs, and prefills ``out`` and the tail of ``ws`` with a sentinel: words
past the written range, and ``ws`` past ``mask_rle_workspace_bytes``, come back unchanged.
"""
import numpy as np
import pytest
import torch

from semantic_segmentation_server_amd.postprocess import mask_rle as MR

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENT = 0x5A5A5A5A
WS_SENT = 0xA5
WS_TAIL = 256


def _hip():
    from semantic_segmentation_server_amd.ops import hip_ops
    return hip_ops


def _launch(lab, out, ws, crop_h, crop_w, cap):
    B, H, W = lab.shape
    _hip().mask_rle(lab, out, ws, B=B, H=H, W=W, crop_h=crop_h, crop_w=crop_w, cap=cap)


def _buffers(B, crop_h, crop_w, cap):
    nb = _hip().mask_rle_workspace_bytes(B, crop_h, crop_w)
    assert nb == B * -(-crop_h * crop_w // _hip().MASK_RLE_CHUNK) * 4
    out = torch.full((B, 4 + cap), SENT, dtype=torch.int32, device=DEV)
    ws = torch.full((nb + WS_TAIL,), WS_SENT, dtype=torch.uint8, device=DEV)
    return out, ws, nb


def _want(labels, crop_h, crop_w, cap):
    return np.stack([MR.encode(l, crop_w, crop_h, cap, out=np.full(4 + cap, SENT, np.uint32))
                     for l in labels])


def _check(labels, crop_h, crop_w, cap):
    """Launch on ``labels`` [B, H, W]; the whole out row (header, runs, untouched sentinel
    words) equals the spec's, the workspace tail is untouched. Returns the device words."""
    labels = np.ascontiguousarray(labels, np.uint8)
    B = labels.shape[0]
    out, ws, nb = _buffers(B, crop_h, crop_w, cap)
    _launch(torch.from_numpy(labels).to(DEV), out, ws, crop_h, crop_w, cap)
    torch.cuda.synchronize()
    got = out.cpu().numpy().view(np.uint32)
    want = _want(labels, crop_h, crop_w, cap)
    for b in range(B):
        used = MR.used_words(want[b])
        assert np.array_equal(got[b, :4], want[b, :4]), (b, got[b, :4], want[b, :4])
        assert np.array_equal(got[b, 4:used], want[b, 4:used]), b
        assert (got[b, used:] == SENT).all(), b
    assert (ws[nb:].cpu().numpy() == WS_SENT).all()
    return got


def _geometric(rng, shape, p=0.02, labels=(0, 1, 20, 127, 128, 255)):
    """A map of random runs (geometric lengths, mean 1 / p) over the flat row-major order."""
    n = int(np.prod(shape))
    lens = rng.geometric(p, size=n // 8 + 8)
    labs = rng.choice(np.asarray(labels, np.uint8), size=len(lens))
    return np.repeat(labs, lens)[:n].reshape(shape)


def test_smaller_than_a_wave_strided_rows():
    rng = np.random.default_rng(1)
    lab = rng.integers(0, 3, (1, 9, 7)).astype(np.uint8)
    lab[0, 1, 1] = 255
    got = _check(lab, 5, 3, 32)
    assert np.array_equal(MR.decode(got[0]), lab[0, :5, :3])


@pytest.mark.parametrize("crop", [(33, 21), (21, 33)])
def test_two_frames_cropped(crop):
    rng = np.random.default_rng(2)
    lab = rng.integers(0, 4, (2, 33, 33)).astype(np.uint8)
    lab[1, 3:9, :] = 255
    got = _check(lab, crop[0], crop[1], 33 * 33)
    for b in range(2):
        assert np.array_equal(MR.decode(got[b]), lab[b, :crop[0], :crop[1]])


@pytest.mark.parametrize("kind", ["start_at_chunk", "straddle"])
def test_chunk_boundary(kind):
    C = _hip().MASK_RLE_CHUNK
    assert 70 * 70 > C
    flat = np.ones(70 * 70, np.uint8)
    flat[100:200] = 7
    flat[C:] = 2
    if kind == "straddle":
        flat[C - 5:C + 7] = 3
    got = _check(flat.reshape(1, 70, 70), 70, 70, 64)
    starts = (got[0, 4:4 + int(got[0, 0])] & 0xFFFFFF).tolist()
    assert (C in starts) == (kind == "start_at_chunk")
    assert ((C - 5) in starts and (C + 7) in starts) == (kind == "straddle")


@pytest.mark.parametrize("cap", [129 * 129, 1000])
@pytest.mark.parametrize("rot", [0, 1, 2])
def test_three_frame_kinds_in_every_position(rot, cap):
    H = W = 129
    N = H * W
    assert -(-N // _hip().MASK_RLE_CHUNK) == 5
    rng = np.random.default_rng(3)
    const = np.full((H, W), 20, np.uint8)
    alt = (np.arange(N) & 1).astype(np.uint8).reshape(H, W) * 255
    geo = _geometric(rng, (H, W))
    frames = [const, alt, geo]
    order = [(i + rot) % 3 for i in range(3)]
    got = _check(np.stack([frames[i] for i in order]), H, W, cap)
    n_geo = int(MR.encode(geo, W, H, N)[0])
    assert 1 < n_geo < 1000
    for pos, kind in enumerate(order):
        assert int(got[pos, 0]) == (1, N, n_geo)[kind]
        if kind == 1 and cap < N:  # truncated: the header still says N, exactly cap entries
            assert MR.used_words(got[pos]) == 4 + cap
            labs, lens, trunc, total = MR.to_wire(got[pos])
            assert trunc and total == N and len(lens) == cap - 1 and int(lens.sum()) == cap - 1
        else:
            assert np.array_equal(MR.decode(got[pos]), frames[kind])


def test_shipped_geometry():
    rng = np.random.default_rng(4)
    coarse = rng.integers(0, 21, (2, 33, 33)).astype(np.uint8)
    lab = np.repeat(np.repeat(coarse, 16, 1), 16, 2)[:, :513, :513]
    got = _check(lab, 385, 513, 16384)
    for b in range(2):
        assert int(got[b, 0]) <= 16384
        assert np.array_equal(MR.decode(got[b]), lab[b, :385, :513])


def test_captured_in_a_graph_and_replayed():
    rng = np.random.default_rng(5)
    H = W = 70
    cap = 512
    maps = [_geometric(rng, (2, H, W), p=0.05), _geometric(rng, (2, H, W), p=0.03)]
    lab = torch.zeros((2, H, W), dtype=torch.uint8, device=DEV)
    out, ws, nb = _buffers(2, 61, 67, cap)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        _launch(lab, out, ws, 61, 67, cap)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        _launch(lab, out, ws, 61, 67, cap)
    for m in maps:
        lab.copy_(torch.from_numpy(m))
        out.fill_(SENT)
        g.replay()
        torch.cuda.synchronize()
        got = out.cpu().numpy().view(np.uint32)
        want = _want(m, 61, 67, cap)
        for b in range(2):
            used = MR.used_words(want[b])
            assert np.array_equal(got[b, :used], want[b, :used])
            assert (got[b, used:] == SENT).all()
    assert (ws[nb:].cpu().numpy() == WS_SENT).all()


def test_copy_to_host_moves_only_the_used_words():
    """mask_rle_copy_to_host: per frame the header and the counted runs land in the pinned
    buffer; everything past them (a truncated frame has nothing past them) keeps the sentinel."""
    H = W = 129
    cap = 1000
    rng = np.random.default_rng(6)
    const = np.full((H, W), 3, np.uint8)
    alt = (np.arange(H * W) & 1).astype(np.uint8).reshape(H, W)
    lab = np.stack([_geometric(rng, (H, W)), alt, const])
    out, ws, _ = _buffers(3, 100, W, cap)
    _launch(torch.from_numpy(lab).to(DEV), out, ws, 100, W, cap)
    host = torch.full((3, 4 + cap), SENT, dtype=torch.int32).pin_memory()
    assert _hip().mask_rle_copy_to_host(out, host) is host
    torch.cuda.synchronize()
    got = host.numpy().view(np.uint32)
    want = _want(lab, 100, W, cap)
    assert [MR.used_words(w) for w in want][1:] == [4 + cap, 5]
    for b in range(3):
        used = MR.used_words(want[b])
        assert np.array_equal(got[b, :used], want[b, :used]), b
        assert (got[b, used:] == SENT).all(), b
    with pytest.raises(ValueError):
        _hip().mask_rle_copy_to_host(out, torch.zeros((3, 4 + cap), dtype=torch.int32))  # not pinned
    with pytest.raises(ValueError):
        _hip().mask_rle_copy_to_host(out, torch.zeros((2, 4 + cap), dtype=torch.int32).pin_memory())
    with pytest.raises(TypeError):
        _hip().mask_rle_copy_to_host(out.float(), host)


def test_wrapper_rejects_bad_arguments_without_launching():
    lab = torch.zeros((1, 9, 7), dtype=torch.uint8, device=DEV)
    out, ws, _ = _buffers(1, 9, 7, 8)
    with pytest.raises(TypeError):
        _launch(lab.to(torch.int32), out, ws, 9, 7, 8)
    with pytest.raises(TypeError):
        _launch(lab, out.float(), ws, 9, 7, 8)
    wide = torch.full((1, 2 * (4 + 8)), SENT, dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError):
        _launch(lab, wide[:, ::2], ws, 9, 7, 8)  # non-contiguous out
    with pytest.raises(ValueError):
        _launch(lab, torch.full((1, 5), SENT, dtype=torch.int32, device=DEV), ws, 9, 7, 1)  # cap < 2
    with pytest.raises(ValueError):
        _launch(lab, out, ws, 10, 7, 8)  # crop > map
    with pytest.raises(ValueError):
        _launch(lab, out, ws, 9, 8, 8)
    with pytest.raises(ValueError):
        _launch(lab, out, ws[:2], 9, 7, 8)  # workspace too small
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == SENT).all() and (wide.cpu().numpy() == SENT).all()


# ---- engine and pipeline -------------------------------------------------------------------

def _cfg(**kw):
    from semantic_segmentation_server_amd import config as C
    base = dict(input_size=129, batch=2, backend="hip", graph=False, min_area_ratio=0.0005)
    base.update(kw)
    return C.Config(**base)


@pytest.mark.parametrize("graph", [False, True])
def test_engine_step_masks_decode_to_its_labels(graph):
    from semantic_segmentation_server_amd.runtime.engine import Engine
    from semantic_segmentation_server_amd.runtime.sources import SyntheticSource
    eng = Engine(_cfg(graph=graph, serve_masks=True, mask_max_runs=4096), torch.device(DEV))
    off = Engine(_cfg(graph=graph), torch.device(DEV))
    assert off.mask_cap == 0
    src = SyntheticSource(200, 150, pool=4, seed=7)
    for k in range(2):
        f, _, _ = src.read_batch(2)
        ids, ts = [2 * k, 2 * k + 1], [1.0, 2.0]
        recs = eng.step(f, ids, ts, [0, 1])
        masks = eng.masks.copy()
        want = eng._infer_eager(torch.from_numpy(f).to(DEV)).cpu().numpy()
        assert masks.shape == (2, 4 + 4096) and masks.dtype == np.uint32
        for b in range(2):
            assert tuple(masks[b, 1:4]) == (eng.crop_w * eng.crop_h, eng.crop_w, eng.crop_h)
            assert np.array_equal(MR.decode(masks[b, :MR.used_words(masks[b])]),
                                  want[b, :eng.crop_h, :eng.crop_w])
        recs_off = off.step(f, ids, ts, [0, 1])
        assert off.masks is None and off.mask_packed is None
        assert recs.dtype == recs_off.dtype and recs.tobytes() == recs_off.tobytes()
    assert off._hip_post.mask_cap == 0 and not off._hip_post._mask_bufs  # no launch, no buffer


def _drive(eng, batches, hub):
    from semantic_segmentation_server_amd.parallel import dist as D
    from semantic_segmentation_server_amd.parallel.dp import DataParallelPipeline
    pipe = DataParallelPipeline(D.init(), eng, 160, 120, 2, "local", hub, 2, lag=2)
    assert pipe.lag == 2 and pipe.nslots == 3 and eng.slot_parallel
    n = len(batches)
    out = []
    pipe.prefetch(batches[0].pin_memory())
    for k in range(n):
        out.append(pipe.step(frame_ids=[100 + 2 * k, 101 + 2 * k], ts=[1.0 + k, 1.5 + k], streams=[0, 1],
                             next_frames=batches[k + 1].pin_memory() if k + 1 < n else None))
    out.append(pipe.flush())
    torch.cuda.synchronize()
    return pipe, np.concatenate(out)


def test_pipeline_pushes_the_latest_mask_of_every_stream():
    from semantic_segmentation_server_amd.runtime.engine import Engine
    from semantic_segmentation_server_amd.runtime.results import ResultHub
    from semantic_segmentation_server_amd.runtime.sources import SyntheticSource
    n = 2 * 3 + 1  # 2 * nslots + 1
    src = SyntheticSource(160, 120, pool=2 * n, seed=11)
    batches = [torch.from_numpy(src.read_batch(2)[0].copy()) for _ in range(n)]
    assert len({b.numpy().tobytes() for b in batches}) == n
    eng = Engine(_cfg(graph=True, serve_masks=True, mask_max_runs=4096), torch.device(DEV))
    hub = ResultHub(2, maxlen=100000)
    pipe, recs = _drive(eng, batches, hub)
    # the slot of the last step still holds its frames: replay it and read its label maps
    labels, _ = eng.run_device(pipe.staging[pipe.slot])
    torch.cuda.synchronize()
    labels = labels.cpu().numpy()
    for s in range(2):
        m = hub.mask(s)
        assert m is not None and m.frame_id == 100 + 2 * (n - 1) + s and m.ts == n + 0.5 * s
        assert len(m.words) == MR.used_words(m.words, 4096)
        assert np.array_equal(MR.decode(m.words), labels[s, :eng.crop_h, :eng.crop_w])
    off = Engine(_cfg(graph=True), torch.device(DEV))
    hub_off = ResultHub(2, maxlen=100000)
    pipe_off, recs_off = _drive(off, batches, hub_off)
    assert pipe_off.local_mask is None and hub_off.mask(0) is None
    assert len(recs) > 0 and recs.tobytes() == recs_off.tobytes()
