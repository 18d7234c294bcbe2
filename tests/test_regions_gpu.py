"""Device class-region kernels (csrc/hip/class_regions.hip) against the numpy definition
(postprocess/regions.py), and the engine / pipeline layers that carry their output.

Every comparison is exact on the uint32 words. ``out`` and the tail of ``ws`` are prefilled
with a sentinel: words past the written range, and ``ws`` past
``class_regions_workspace_bytes``, come back unchanged. The shapes derive from the tile the
wrapper exports: a crop of 3 x 3 tiles with ragged right and bottom edges, narrower than the
map (pitch != width).
"""
import functools

import numpy as np
import pytest
import torch

from semantic_segmentation_server_amd.postprocess import regions as RG

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENT = 0x5A5A5A5A
WS_SENT = 0xA5
WS_TAIL = 256


def _hip():
    from semantic_segmentation_server_amd.ops import hip_ops
    return hip_ops


def _geom():
    """(H, W, crop_h, crop_w, tile_h, tile_w): 97 x 73 crop of a 101 x 97 map for a 32 x 32 tile."""
    tw, th = _hip().REGION_TILE_W, _hip().REGION_TILE_H
    cw, ch = 3 * tw + 1, 2 * th + 9
    return 3 * th + 1, cw + 4, ch, cw, th, tw


def _launch(lab, out, ws, crop_h, crop_w, classes, min_pixels, K):
    B, H, W = lab.shape
    _hip().class_regions(lab, out, ws, B=B, H=H, W=W, crop_h=crop_h, crop_w=crop_w,
                         classes=classes, min_pixels=min_pixels, K=K)


def _buffers(B, crop_h, crop_w, K):
    nb = _hip().class_regions_workspace_bytes(B, crop_h, crop_w)
    out = torch.full((B, 4 + 6 * K), SENT, dtype=torch.int32, device=DEV)
    ws = torch.full((nb + WS_TAIL,), WS_SENT, dtype=torch.uint8, device=DEV)
    return out, ws, nb


def _want(labels, crop_h, crop_w, classes, min_pixels, K):
    return np.stack([RG.encode(l, crop_w, crop_h, classes, min_pixels, K,
                               out=np.full(4 + 6 * K, SENT, np.uint32)) for l in labels])


def _check(labels, crop_h, crop_w, classes, min_pixels=2, K=16, want=None):
    """Launch on ``labels`` [B, H, W]: the whole out row (header, records, untouched sentinel
    words) equals the definition's and the workspace tail is untouched. Returns the regions
    of every frame, decoded."""
    labels = np.ascontiguousarray(labels, np.uint8)
    B = labels.shape[0]
    out, ws, nb = _buffers(B, crop_h, crop_w, K)
    _launch(torch.from_numpy(labels).to(DEV), out, ws, crop_h, crop_w, classes, min_pixels, K)
    torch.cuda.synchronize()
    got = out.cpu().numpy().view(np.uint32)
    if want is None:
        want = _want(labels, crop_h, crop_w, classes, min_pixels, K)
    for b in range(B):
        assert np.array_equal(got[b, :4], want[b, :4]), (b, got[b, :4], want[b, :4])
        assert np.array_equal(got[b], want[b]), (b, np.flatnonzero(got[b] != want[b])[:8])
    assert (ws[nb:].cpu().numpy() == WS_SENT).all()
    return [RG.decode(g) for g in got]


def _canvas(fill=0, B=1):
    H, W = _geom()[:2]
    return np.full((B, H, W), fill, np.uint8)


def test_one_giant_region():
    H, W, ch, cw, _, _ = _geom()
    (t,) = _check(_canvas(5), ch, cw, [5])
    assert len(t) == 1 and t[0]["pixels"] == ch * cw and t[0]["root"] == 0 and t[0]["label"] == 5
    assert (t[0]["x_min"], t[0]["y_min"], t[0]["x_max"], t[0]["y_max"]) == (0, 0, cw - 1, ch - 1)


def test_checkerboard_is_two_regions_through_the_diagonals():
    H, W, ch, cw, _, _ = _geom()
    y, x = np.mgrid[:H, :W]
    (t,) = _check((1 + ((x + y) & 1)).astype(np.uint8)[None], ch, cw, [1, 2])
    n = ch * cw
    assert t["pixels"].tolist() == [(n + 1) // 2, n // 2] and t["root"].tolist() == [0, 1]


def test_all_singletons():
    hip = _hip()
    cw = 2 * hip.REGION_TILE_W + 1
    ch = hip.REGION_CANDIDATES // cw
    n = cw * ch
    assert n <= hip.REGION_CANDIDATES and ch > hip.REGION_TILE_H
    y, x = np.mgrid[:ch + 2, :cw + 3]
    lab = (1 + (x & 1) + 2 * (y & 1)).astype(np.uint8)
    K = 64
    want = np.full((1, 4 + 6 * K), SENT, np.uint32)  # written out by hand: pixel i is region i
    want[0, :4] = (n, n, cw, ch)
    for i in range(K):
        px, py = i % cw, i // cw
        want[0, 4 + 6 * i:10 + 6 * i] = ((int(lab[py, px]) << 24) | i, 1, px, py,
                                         px | (py << 16), px | (py << 16))
    (t,) = _check(lab[None], ch, cw, [1, 2, 3, 4], 1, K, want=want)
    assert len(t) == K and (t["pixels"] == 1).all() and t["root"].tolist() == list(range(K))
    assert np.array_equal(want, _want(lab[None], ch, cw, [1, 2, 3, 4], 1, K))


@pytest.mark.parametrize("transposed", [False, True])
def test_serpentine_is_one_region(transposed):
    """A one-pixel-wide path along every other row (column), joined at alternating ends: it
    crosses every tile many times and its unions form long chains."""
    H, W, ch, cw, _, _ = _geom()
    lab = _canvas(0)[0]
    if transposed:
        lab[:ch, 0:cw:2] = 3
        for k, x in enumerate(range(1, cw - 1, 2)):
            lab[ch - 1 if k % 2 == 0 else 0, x] = 3
        on = ch * ((cw + 1) // 2) + len(range(1, cw - 1, 2))
    else:
        lab[0:ch:2, :cw] = 3
        for k, y in enumerate(range(1, ch - 1, 2)):
            lab[y, cw - 1 if k % 2 == 0 else 0] = 3
        on = cw * ((ch + 1) // 2) + len(range(1, ch - 1, 2))
    lab[ch:, :] = 3  # outside the crop: ignored
    lab[:, cw:] = 3
    (t,) = _check(lab[None], ch, cw, [3])
    assert len(t) == 1 and t[0]["pixels"] == on and t[0]["root"] == 0


def _corner_blobs(anti):
    """Two 6 x 6 blobs of class 1 on class 2, touching only by one diagonal step across the
    corner where four tiles meet."""
    _, _, _, _, th, tw = _geom()
    lab = _canvas(2)[0]
    if anti:
        lab[th - 6:th, tw:tw + 6] = 1
        lab[th:th + 6, tw - 6:tw] = 1
    else:
        lab[th - 6:th, tw - 6:tw] = 1
        lab[th:th + 6, tw:tw + 6] = 1
    return lab


@pytest.mark.parametrize("anti", [False, True])
def test_corner_link_joins_two_blobs(anti):
    _, _, ch, cw, _, _ = _geom()
    (t,) = _check(_corner_blobs(anti)[None], ch, cw, [1, 2])
    ones = t[t["label"] == 1]
    assert len(t) == 2 and len(ones) == 1 and ones[0]["pixels"] == 72


@pytest.mark.parametrize("anti", [False, True])
def test_an_excluded_class_separates_them(anti):
    _, _, ch, cw, th, tw = _geom()
    lab = _corner_blobs(anti)
    lab[th, tw - 1 if anti else tw] = 9  # the linking pixel of the lower blob: class 9 is not served
    (t,) = _check(lab[None], ch, cw, [1, 2])
    ones = t[t["label"] == 1]
    assert sorted(ones["pixels"].tolist()) == [35, 36] and not (t["label"] == 9).any()


def _blob_frame(seed):
    H, W = _geom()[:2]
    rng = np.random.default_rng(seed)
    coarse = rng.integers(0, 6, (H // 8 + 1, W // 8 + 1)).astype(np.uint8)
    lab = np.repeat(np.repeat(coarse, 8, 0), 8, 1)[:H, :W].copy()
    sp = rng.random((H, W)) < 0.03
    lab[sp] = rng.integers(0, 6, int(sp.sum()))
    return lab


@pytest.mark.parametrize("rot", [0, 1, 2])
def test_three_frame_kinds_in_every_position(rot):
    H, W, ch, cw, _, _ = _geom()
    y, x = np.mgrid[:H, :W]
    frames = [_canvas(5)[0], (1 + ((x + y) & 1)).astype(np.uint8), _blob_frame(3)]
    order = [(i + rot) % 3 for i in range(3)]
    tabs = _check(np.stack([frames[i] for i in order]), ch, cw, [1, 2, 3, 4, 5], 4, 32)
    for pos, kind in enumerate(order):
        if kind < 2:
            assert len(tabs[pos]) == (1, 2)[kind]
        else:
            assert len(tabs[pos]) > 4


def _squares():
    """Eight 5 x 5 squares of classes 1 / 2 in different tiles, one of them across a tile
    corner, and one 7 x 7; class 0 around them is not served."""
    _, _, ch, cw, th, tw = _geom()
    lab = _canvas(0)[0]
    at = [(2, 3), (2, tw + 4), (th + 3, 2 * tw + 8), (th - 2, tw - 3), (2 * th + 1, 5),
          (th + 9, 3), (3, 2 * tw + 20), (2 * th + 3, 3 * tw - 4)]
    for k, (y, x) in enumerate(at):
        assert y + 5 <= ch and x + 5 <= cw
        lab[y:y + 5, x:x + 5] = 1 + (k & 1)
    lab[th + 8:th + 15, tw + 8:tw + 15] = 2
    return lab, at


def test_area_ties_are_ordered_by_root():
    _, _, ch, cw, _, _ = _geom()
    lab, at = _squares()
    (t,) = _check(lab[None], ch, cw, [1, 2], 25, 16)
    assert t["pixels"].tolist() == [49] + [25] * 8
    assert t["root"].tolist()[1:] == sorted(y * cw + x for y, x in at)


def test_cut_off_keeps_the_true_count_and_k_records():
    _, _, ch, cw, _, _ = _geom()
    lab, at = _squares()
    out, ws, _ = _buffers(1, ch, cw, 3)
    _launch(torch.from_numpy(lab[None]).to(DEV), out, ws, ch, cw, [1, 2], 25, 3)
    got = out.cpu().numpy().view(np.uint32)[0]
    assert got[0] == 9 and RG.used_words(got) == 4 + 18 and len(RG.decode(got)) == 3
    _check(lab[None], ch, cw, [1, 2], 25, 3)
    (t,) = _check(lab[None], ch, cw, [1, 2], 26, 3)  # min_pixels drops the 25-pixel squares
    assert t["pixels"].tolist() == [49]


@functools.lru_cache(maxsize=None)
def _shipped():
    rng = np.random.default_rng(4)
    coarse = rng.integers(0, 21, (2, 33, 33)).astype(np.uint8)
    lab = np.repeat(np.repeat(coarse, 16, 1), 16, 2)[:, :513, :513].copy()
    sp = rng.random(lab.shape) < 0.02
    lab[sp] = rng.integers(0, 21, int(sp.sum()))
    mp = RG.min_pixels_for(0.002, 513, 513)
    want = _want(lab, 385, 513, RG.default_classes(21), mp, 64)
    want.setflags(write=False)
    return lab, mp, want


def test_shipped_geometry():
    lab, mp, want = _shipped()
    tabs = _check(lab, 385, 513, RG.default_classes(21), mp, 64, want=want)
    assert all(len(t) > 8 for t in tabs)


def test_captured_in_a_graph_and_replayed_on_new_labels():
    H, W, ch, cw, _, _ = _geom()
    K, cls, mp = 16, [1, 2, 3, 4, 5], 6
    maps = [np.stack([_blob_frame(5), _squares()[0]]), np.stack([_canvas(5)[0], _blob_frame(6)])]
    lab = torch.zeros((2, H, W), dtype=torch.uint8, device=DEV)
    out, ws, nb = _buffers(2, ch, cw, K)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        _launch(lab, out, ws, ch, cw, cls, mp, K)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        _launch(lab, out, ws, ch, cw, cls, mp, K)
    for m in maps:
        lab.copy_(torch.from_numpy(m))
        out.fill_(SENT)
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy().view(np.uint32), _want(m, ch, cw, cls, mp, K))
    assert (ws[nb:].cpu().numpy() == WS_SENT).all()


def test_wrapper_rejects_bad_arguments_without_launching():
    lab = torch.zeros((1, 9, 7), dtype=torch.uint8, device=DEV)
    out, ws, _ = _buffers(1, 9, 7, 8)
    ok = dict(crop_h=9, crop_w=7, classes=[1], min_pixels=1, K=8)

    def go(lab=lab, out=out, ws=ws, **kw):
        a = dict(ok)
        a.update(kw)
        _launch(lab, out, ws, a["crop_h"], a["crop_w"], a["classes"], a["min_pixels"], a["K"])

    with pytest.raises(TypeError):
        go(lab=lab.to(torch.int32))
    with pytest.raises(TypeError):
        go(out=out.float())
    wide = torch.full((1, 2 * (4 + 48)), SENT, dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError):
        go(out=wide[:, ::2])  # non-contiguous out
    with pytest.raises(ValueError):
        go(crop_h=10)  # crop > map
    with pytest.raises(ValueError):
        go(crop_w=8)
    with pytest.raises(ValueError):
        go(ws=ws[:16])  # workspace too small
    with pytest.raises(ValueError):
        go(K=0)
    with pytest.raises(ValueError):
        go(K=257, out=torch.full((1, 4 + 6 * 257), SENT, dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError):
        go(K=7)  # out is shaped for K = 8
    with pytest.raises(ValueError):
        go(min_pixels=0)
    with pytest.raises(ValueError):
        go(classes=[256])
    big = torch.zeros((1, 80, 80), dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError):  # 6400 pixels, min_pixels 1: more than REGION_CANDIDATES could pass
        _launch(big, out, torch.zeros(_hip().class_regions_workspace_bytes(1, 80, 80), dtype=torch.uint8,
                                      device=DEV), 80, 80, [1], 1, 8)
    many = torch.zeros((65536, 1, 1), dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError):
        _launch(many, torch.full((65536, 4 + 48), SENT, dtype=torch.int32, device=DEV), ws, 1, 1, [1], 1, 8)
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == SENT).all() and (wide.cpu().numpy() == SENT).all()
    assert (ws.cpu().numpy() == WS_SENT).all()


# ---- engine and pipeline -------------------------------------------------------------------

def _cfg(**kw):
    from semantic_segmentation_server_amd import config as C
    base = dict(input_size=129, batch=2, backend="hip", graph=False, min_area_ratio=0.0005)
    base.update(kw)
    return C.Config(**base)


def _want_engine(eng, labels):
    return np.stack([RG.encode(l, eng.crop_w, eng.crop_h, eng.region_mask, eng.region_min_pixels,
                               eng.region_cap) for l in labels])


@pytest.mark.parametrize("graph", [False, True])
def test_engine_step_regions_are_those_of_its_labels(graph):
    from semantic_segmentation_server_amd.runtime.engine import Engine
    from semantic_segmentation_server_amd.runtime.sources import SyntheticSource
    eng = Engine(_cfg(graph=graph, serve_regions=True), torch.device(DEV))
    off = Engine(_cfg(graph=graph), torch.device(DEV))
    assert off.region_cap == 0 and eng.region_cap == 64
    assert eng.region_min_pixels == int(np.ceil(0.002 * 129 * 129))
    src = SyntheticSource(200, 150, pool=4, seed=7)
    for k in range(2):
        f, _, _ = src.read_batch(2)
        ids, ts = [2 * k, 2 * k + 1], [1.0, 2.0]
        recs = eng.step(f, ids, ts, [0, 1])
        got = eng.regions.copy()
        labels = eng._infer_eager(torch.from_numpy(f).to(DEV)).cpu().numpy()
        assert got.shape == (2, 4 + 6 * 64) and got.dtype == np.uint32
        want = _want_engine(eng, labels)
        for b in range(2):
            used = RG.used_words(want[b])
            assert np.array_equal(got[b, :used], want[b, :used]), b
        recs_off = off.step(f, ids, ts, [0, 1])
        assert off.regions is None and off.region_packed is None
        assert recs.dtype == recs_off.dtype and recs.tobytes() == recs_off.tobytes()
    assert off._hip_post.region_cap == 0 and not off._hip_post._region_bufs  # no launch, no buffer


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


def _batches(n):
    from semantic_segmentation_server_amd.runtime.sources import SyntheticSource
    src = SyntheticSource(160, 120, pool=2 * n, seed=11)
    batches = [torch.from_numpy(src.read_batch(2)[0].copy()) for _ in range(n)]
    assert len({b.numpy().tobytes() for b in batches}) == n
    return batches


def test_pipeline_pushes_the_latest_regions_of_every_stream():
    from semantic_segmentation_server_amd.runtime.engine import Engine
    from semantic_segmentation_server_amd.runtime.results import ResultHub
    n = 2 * 3 + 1  # 2 * nslots + 1
    batches = _batches(n)
    eng = Engine(_cfg(graph=True, serve_regions=True), torch.device(DEV))
    hub = ResultHub(2, maxlen=100000)
    pipe, recs = _drive(eng, batches, hub)
    # the slot of the last step still holds its frames: replay it and read its label maps
    labels, _ = eng.run_device(pipe.staging[pipe.slot])
    torch.cuda.synchronize()
    want = _want_engine(eng, labels.cpu().numpy())
    for s in range(2):
        r = hub.regions(s)
        assert r is not None and r.frame_id == 100 + 2 * (n - 1) + s and r.ts == n + 0.5 * s
        assert len(r.words) == RG.used_words(want[s])
        assert np.array_equal(r.words, want[s][:len(r.words)])
    off = Engine(_cfg(graph=True), torch.device(DEV))
    hub_off = ResultHub(2, maxlen=100000)
    pipe_off, recs_off = _drive(off, batches, hub_off)
    assert pipe_off.local_regions is None and hub_off.regions(0) is None
    assert len(recs) > 0 and recs.tobytes() == recs_off.tobytes()


def test_masks_and_regions_together_match_their_own_oracles():
    from semantic_segmentation_server_amd.postprocess import mask_rle as MR
    from semantic_segmentation_server_amd.runtime.engine import Engine
    from semantic_segmentation_server_amd.runtime.results import ResultHub
    batches = _batches(4)
    eng = Engine(_cfg(graph=True, serve_regions=True, serve_masks=True, mask_max_runs=4096,
                      max_regions=8, region_classes="person,7,0"), torch.device(DEV))
    assert eng.region_cap == 8 and eng.region_mask == (1 << 15) | (1 << 7) | 1
    hub = ResultHub(2, maxlen=100000)
    pipe, _ = _drive(eng, batches, hub)
    labels, _ = eng.run_device(pipe.staging[pipe.slot])
    torch.cuda.synchronize()
    labels = labels.cpu().numpy()
    want = _want_engine(eng, labels)
    for s in range(2):
        r, m = hub.regions(s), hub.mask(s)
        assert r.frame_id == m.frame_id == 100 + 2 * 3 + s
        assert np.array_equal(r.words, want[s][:RG.used_words(want[s])])
        assert np.array_equal(MR.decode(m.words), labels[s, :eng.crop_h, :eng.crop_w])
