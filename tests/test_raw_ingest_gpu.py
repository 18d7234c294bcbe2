"""Raw 4:2:2 ingest on the GPU: the conversion kernel (csrc/hip/yuv422.hip) against the host
conversion (csrc/host/v4l2.cpp) byte for byte in every alignment case, and engines and a
pipeline that ingest packed frames against default ones stepped on the host-converted BGR."""
import numpy as np
import pytest
import torch

from raw_ingest_ref import exhaustive_stream, host_bgr

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENT = 0xA5
GUARD = 64  # sentinel bytes kept after (and, for a slice, before) the written range


def _hip():
    from semantic_segmentation_server_amd.ops import hip_ops
    return hip_ops


def _out(shape):
    """(an `out` of `shape` inside a sentinel-filled allocation, the allocation)."""
    n = int(np.prod(shape))
    store = torch.full((n + GUARD,), SENT, dtype=torch.uint8, device=DEV)
    return store[:n].view(shape), store


def _check(x: np.ndarray):
    """Both byte orders of `x` (B, H, W, 2): kernel == host, guard bytes untouched."""
    src = torch.from_numpy(x).to(DEV)
    for uyvy in (False, True):
        out, store = _out(x.shape[:3] + (3,))
        assert _hip().yuv422_to_bgr(src, out, uyvy=uyvy) is out
        torch.cuda.synchronize()
        assert torch.equal(out.cpu(), torch.from_numpy(host_bgr(x, uyvy))), uyvy
        assert (store[out.numel():] == SENT).all()


def test_one_macropixel():
    _check(np.array([[[[81, 90], [210, 240]]]], np.uint8))
    _check(np.random.default_rng(0).integers(0, 256, (1, 1, 2, 2), dtype=np.uint8))


def test_misaligned_frames_and_a_batch_slice():
    x = np.random.default_rng(1).integers(0, 256, (3, 3, 6, 2), dtype=np.uint8)
    _check(x)  # 36 B in, 54 B out per frame: 27 macropixels, not a multiple of 8
    src = torch.from_numpy(x).to(DEV)
    for uyvy in (False, True):
        out, store = _out((3, 3, 6, 3))
        _hip().yuv422_to_bgr(src[1:3], out[1:3], uyvy=uyvy)  # starts 36 B / 54 B into the buffers
        torch.cuda.synchronize()
        assert (out[0] == SENT).all() and (store[out.numel():] == SENT).all()
        assert torch.equal(out[1:3].cpu(), torch.from_numpy(host_bgr(x[1:3], uyvy)))
        out, store = _out((3, 3, 6, 3))
        _hip().yuv422_to_bgr(src[2:3], out[2:3], uyvy=uyvy)  # 72 B / 108 B: 8 B and 12 B off the grid
        torch.cuda.synchronize()
        assert (out[:2] == SENT).all() and (store[out.numel():] == SENT).all()
        assert torch.equal(out[2].cpu(), torch.from_numpy(host_bgr(x[2], uyvy)))


def test_vector_body_and_tail_in_every_alignment_phase():
    x = np.random.default_rng(2).integers(0, 256, (2, 5, 34, 2), dtype=np.uint8)
    _check(x)  # 170 macropixels: 21 groups of 8 and a tail of 2
    # every start phase: a source 4 k bytes and a destination 6 k bytes into aligned buffers
    # (k = 0..7: heads of 0..7 macropixels), and sources whose phase disagrees with the
    # destination's (the narrow path for the whole stream)
    flat = x.reshape(-1, 4)
    n = len(flat)
    src = torch.from_numpy(flat).to(DEV)
    for k in range(8):
        for skew in (0, 1):
            m = n - k - skew
            s = src[k + skew:].reshape(1, 1, 2 * m, 2)
            store = torch.full((6 * n + GUARD,), SENT, dtype=torch.uint8, device=DEV)
            out = store[6 * k:6 * (k + m)].view(1, 1, 2 * m, 3)
            _hip().yuv422_to_bgr(s, out, uyvy=bool(k & 1))
            torch.cuda.synchronize()
            want = host_bgr(flat[k + skew:].reshape(1, 1, 2 * m, 2), bool(k & 1))
            assert torch.equal(out.cpu(), torch.from_numpy(want)), (k, skew)
            assert (store[:6 * k] == SENT).all() and (store[6 * (k + m):] == SENT).all(), (k, skew)


@pytest.fixture(scope="module")
def exhaustive():
    s = exhaustive_stream()
    return s, torch.from_numpy(s).to(DEV)


@pytest.mark.parametrize("uyvy", [False, True])
def test_exhaustive(exhaustive, uyvy):
    s, src = exhaustive
    out, store = _out((1, 4096, 8192, 3))
    _hip().yuv422_to_bgr(src.view(1, 4096, 8192, 2), out, uyvy=uyvy)
    torch.cuda.synchronize()
    want = torch.from_numpy(host_bgr(s, uyvy)).to(DEV)
    assert torch.equal(out[0], want)
    assert (store[out.numel():] == SENT).all()


def test_shipped_geometry():
    _check(np.random.default_rng(3).integers(0, 256, (2, 480, 640, 2), dtype=np.uint8))


def test_captured_in_a_graph_and_replayed():
    rng = np.random.default_rng(4)
    xs = [rng.integers(0, 256, (2, 6, 10, 2), dtype=np.uint8) for _ in range(2)]
    src = torch.zeros((2, 6, 10, 2), dtype=torch.uint8, device=DEV)
    out, store = _out((2, 6, 10, 3))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        _hip().yuv422_to_bgr(src, out)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        _hip().yuv422_to_bgr(src, out)
    for x in xs:
        src.copy_(torch.from_numpy(x))
        store.fill_(SENT)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out.cpu(), torch.from_numpy(host_bgr(x, False)))
        assert (store[out.numel():] == SENT).all()


def test_wrapper_refuses_bad_arguments_without_launching():
    f = _hip().yuv422_to_bgr
    src = torch.zeros((1, 4, 6, 2), dtype=torch.uint8, device=DEV)
    out, store = _out((1, 4, 6, 3))
    odd, odd_store = _out((1, 4, 5, 3))
    wide = torch.full((1, 4, 6, 6), SENT, dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError):
        f(torch.zeros((1, 4, 5, 2), dtype=torch.uint8, device=DEV), odd)  # odd W
    with pytest.raises(TypeError):
        f(src.to(torch.int32), out)
    with pytest.raises(TypeError):
        f(src, out.to(torch.int32))
    with pytest.raises(ValueError):
        f(src, wide[..., ::2])  # non-contiguous out
    with pytest.raises(ValueError):
        f(src, out.view(1, 6, 4, 3))  # wrong out shape
    with pytest.raises(ValueError):
        f(src, out.view(4, 6, 3))
    with pytest.raises(ValueError):
        f(torch.zeros((1, 4, 6, 3), dtype=torch.uint8, device=DEV), out)  # BGR as the source
    with pytest.raises(ValueError):
        f(src.cpu(), out)
    with pytest.raises(ValueError):
        f(src, torch.zeros((1, 4, 6, 3), dtype=torch.uint8))
    torch.cuda.synchronize()
    for t in (store, odd_store, wide):
        assert (t == SENT).all()


# ---- engine and pipeline -------------------------------------------------------------------

def _cfg(**kw):
    from semantic_segmentation_server_amd import config as C
    base = dict(input_size=129, batch=2, backend="hip", graph=False, min_area_ratio=0.0005)
    base.update(kw)
    return C.Config(**base)


@pytest.fixture
def one_plan(monkeypatch, tmp_path):
    """The two HIP engines of a comparison run the same kernels. No committed plan covers the
    small test shape, so each engine would pick its kernel variants by timing them, and
    variants differ in rounding (models/plan.py): with SSA_TUNE_FILE the first engine's picks
    are written to a file and the second engine reads them."""
    monkeypatch.setenv("SSA_TUNE_FILE", str(tmp_path / "tune.json"))


def _engines(fmt, **kw):
    from semantic_segmentation_server_amd.runtime.engine import Engine
    return Engine(_cfg(pixel_format=fmt, **kw), torch.device(DEV)), Engine(_cfg(**kw), torch.device(DEV))


def _step_both(eng, ref, fmt):
    from semantic_segmentation_server_amd.runtime.sources import SyntheticSource
    assert (eng.frame_channels, ref.frame_channels) == (2, 3)
    src = SyntheticSource(200, 150, pool=4, seed=7, pixel_format=fmt)
    for k in range(2):
        raw, _, _ = src.read_batch(2)
        bgr = host_bgr(raw, fmt == "uyvy")
        ids, ts = [2 * k, 2 * k + 1], [1.0, 2.0]
        recs = eng.step(raw, ids, ts, [0, 1])
        want = ref.step(bgr, ids, ts, [0, 1])
        assert len(want) > 0 and recs.dtype == want.dtype and recs.tobytes() == want.tobytes()
        with torch.no_grad():
            assert torch.equal(eng._infer_eager(torch.from_numpy(raw).to(DEV)),
                               ref._infer_eager(torch.from_numpy(bgr).to(DEV)))


@pytest.mark.parametrize("fmt", ["yuyv", "uyvy"])
@pytest.mark.parametrize("graph", [False, True])
def test_engine_step_equals_a_bgr_engine_on_converted_frames(one_plan, graph, fmt):
    eng, ref = _engines(fmt, graph=graph)
    _step_both(eng, ref, fmt)
    if graph:  # the static step owns the BGR frames its model read
        assert tuple(eng._static_step.frames.shape) == (2, 150, 200, 2)
        assert tuple(eng._static_step.bgr.shape) == (2, 150, 200, 3)


def test_engine_step_on_the_torch_backend(monkeypatch):
    """The stock-PyTorch path converts with the torch definition. Its bf16 convolutions are not
    run-to-run reproducible by default (measured on the MI355X: one engine, one input, ten
    calls, two different label maps, logits 0.0625 apart); with deterministic algorithms
    selected they are, and two engines can be compared exactly."""
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    _step_both(*_engines("yuyv", backend="torch", graph=False), "yuyv")


def _drive(eng, batches):
    from semantic_segmentation_server_amd.parallel import dist as D
    from semantic_segmentation_server_amd.parallel.dp import DataParallelPipeline
    pipe = DataParallelPipeline(D.init(), eng, 160, 120, 2, "local", None, 2, lag=2)
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


def test_pipeline_on_raw_batches_equals_a_bgr_pipeline(one_plan):
    from semantic_segmentation_server_amd.runtime.sources import SyntheticSource
    n = 2 * 3 + 1  # 2 * nslots + 1
    src = SyntheticSource(160, 120, pool=2 * n, seed=11, pixel_format="yuyv")
    raw = [src.read_batch(2)[0].copy() for _ in range(n)]
    assert len({b.tobytes() for b in raw}) == n
    eng, ref = _engines("yuyv", graph=True)
    pipe, recs = _drive(eng, [torch.from_numpy(b) for b in raw])
    assert pipe.staging[0].shape[-1] == 2 and tuple(pipe.staging[2].shape) == (2, 120, 160, 2)
    steps = list(eng._bound_graphs.values())
    assert len(steps) == 3 and all(tuple(s.bgr.shape) == (2, 120, 160, 3) for s in steps)
    # the slot of the last step still holds its BGR frames
    last = eng._bound_graphs[pipe.staging[pipe.slot].data_ptr()]
    assert torch.equal(last.bgr.cpu(), torch.from_numpy(host_bgr(raw[-1], False)))
    pipe_ref, want = _drive(ref, [torch.from_numpy(host_bgr(b, False)) for b in raw])
    assert pipe_ref.staging[0].shape[-1] == 3
    assert len(want) > 0 and recs.dtype == want.dtype and recs.tobytes() == want.tobytes()


def test_default_engine_converts_nothing():
    from semantic_segmentation_server_amd.runtime.engine import Engine
    from semantic_segmentation_server_amd.runtime.sources import SyntheticSource
    eng = Engine(_cfg(graph=True), torch.device(DEV))
    assert eng.frame_channels == 3 and eng.pixel_format == "bgr"
    f, _, _ = SyntheticSource(200, 150, pool=2, seed=7).read_batch(2)
    eng.step(f, [0, 1], [1.0, 2.0], [0, 1])
    fd = torch.from_numpy(f).to(DEV)
    assert eng.to_bgr(fd) is fd and eng.bgr_buffer(fd) is None
    assert eng._static_step.bgr is None and tuple(eng._static_step.frames.shape) == (2, 150, 200, 3)
