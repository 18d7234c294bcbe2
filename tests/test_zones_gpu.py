"""Device zone-occupancy kernel (csrc/hip/zone_stats.hip) against the numpy definition
(postprocess/zones.py), and the engine / pipeline layers that carry its output.

Every comparison is exact on the uint32 words, and on the whole row: ``out`` is prefilled with
a sentinel (every word must be written) and ``ws`` is over-allocated by a sentinel tail that
must come back unchanged. The base geometry derives from the chunk the wrapper exports: a crop
of a little over two chunks of flat pixels with an odd width, inside a larger map of odd width
(rows are not 4-byte aligned) whose pixels outside the crop hold a served class, so a read past
the crop shows up in the counts.
"""
import json

import numpy as np
import pytest
import torch

from semantic_segmentation_server_amd.postprocess import zones as ZN

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENT = 0x5A5A5A5A
WS_SENT = 0xA5
WS_TAIL = 256
OUTSIDE = 1  # the class of every pixel outside the crop


def _hip():
    from semantic_segmentation_server_amd.ops import hip_ops
    return hip_ops


def _geom():
    """(H, W, crop_h, crop_w, chunk): a crop of 97 columns and a little over 2 chunks of flat
    pixels inside a map 3 rows taller and 4 columns wider (odd width)."""
    chunk = _hip().zone_stats_chunk()
    cw = 97
    ch = -(-(2 * chunk + 9) // cw)
    assert cw * ch >= 2 * chunk + 9 and (cw + 4) % 2 == 1
    return ch + 3, cw + 4, ch, cw, chunk


def _canvas(inner, crop_h, crop_w, H=None, W=None):
    """[B, H, W] uint8: ``inner`` ([B, crop_h, crop_w]) inside a map filled with OUTSIDE."""
    inner = np.asarray(inner, np.uint8)
    if inner.ndim == 2:
        inner = inner[None]
    H, W = H or crop_h + 3, W or crop_w + 4
    lab = np.full((inner.shape[0], H, W), OUTSIDE, np.uint8)
    lab[:, :crop_h, :crop_w] = inner
    return lab


def _want(labels, plane, crop_h, crop_w, R, C, conf=None):
    return np.stack([ZN.encode(labels[b], plane, crop_w, crop_h, C, rows=R,
                               conf=None if conf is None else conf[b]) for b in range(len(labels))])


def _buffers(B, R, C, conf):
    nb = _hip().zone_stats_workspace_bytes(B, R, C, conf)
    out = torch.full((B, ZN.frame_words(R, C, conf)), SENT, dtype=torch.int32, device=DEV)
    ws = torch.full((nb + WS_TAIL,), WS_SENT, dtype=torch.uint8, device=DEV)
    return out, ws, nb


def _dev_plane(plane):
    return None if plane is None else torch.from_numpy(np.ascontiguousarray(plane, np.uint32).view(np.int32)).to(DEV)


def _check(labels, plane, crop_h, crop_w, R, C, conf=None, want=None):
    """Launch on ``labels`` [B, H, W] (and ``conf``): every word of every row equals the
    definition's and the workspace tail is untouched. Returns the decoded frames."""
    labels = np.ascontiguousarray(labels, np.uint8)
    B, H, W = labels.shape
    out, ws, nb = _buffers(B, R, C, conf is not None)
    cf = None if conf is None else torch.from_numpy(np.ascontiguousarray(conf, np.uint8)).to(DEV)
    _hip().zone_stats(torch.from_numpy(labels).to(DEV), out, ws, B=B, H=H, W=W, crop_h=crop_h,
                      crop_w=crop_w, R=R, C=C, plane=_dev_plane(plane), conf=cf)
    torch.cuda.synchronize()
    got = out.cpu().numpy().view(np.uint32)
    if want is None:
        want = _want(labels, plane, crop_h, crop_w, R, C, conf)
    for b in range(B):
        assert np.array_equal(got[b, :4], want[b, :4]), (b, got[b, :4], want[b, :4])
        assert np.array_equal(got[b], want[b]), (b, np.flatnonzero(got[b] != want[b])[:8])
    assert (ws[nb:].cpu().numpy() == WS_SENT).all()
    return [ZN.decode(g, conf=conf is not None) for g in got]


def _blocks(rng, crop_h, crop_w, C, speckle=0.02):
    """Piecewise-constant labels (random rectangles) plus speckle, all < C."""
    lab = np.full((crop_h, crop_w), rng.integers(C), np.uint8)
    for _ in range(6):
        y0, x0 = rng.integers(crop_h), rng.integers(crop_w)
        lab[y0:y0 + 1 + rng.integers(crop_h), x0:x0 + 1 + rng.integers(crop_w)] = rng.integers(C)
    m = rng.random((crop_h, crop_w)) < speckle
    lab[m] = rng.integers(C, size=int(m.sum()))
    return lab


# ---- kernel ---------------------------------------------------------------------------------

def test_one_class_in_all_32_zones_everywhere():
    """Maximum contention: every run adds to 33 counters, and every counter equals N."""
    H, W, ch, cw, _ = _geom()
    plane = np.full((ch, cw), 0xFFFFFFFF, np.uint32)
    conf = np.full((1, H, W), 255, np.uint8)
    (t,) = _check(_canvas(np.full((ch, cw), 7, np.uint8), ch, cw, H, W), plane, ch, cw, 33, 21, conf)
    n = ch * cw
    assert (t.pixels[:, 7] == n).all() and t.pixels.sum() == 33 * n
    assert (t.sum_conf[:, 7] == 255 * n).all()


def test_checkerboard_against_striped_zones_has_no_runs():
    H, W, ch, cw, _ = _geom()
    y, x = np.mgrid[:ch, :cw]
    lab = (2 + ((x + y) & 1)).astype(np.uint8)
    plane = ((x % 3 == 0) | ((x % 3 == 1) << 1) | ((y % 2) << 2) | (((x + 2 * y) % 5 == 0) << 3)).astype(np.uint32)
    rng = np.random.default_rng(1)
    conf = rng.integers(0, 256, (1, H, W), dtype=np.uint8)
    _check(_canvas(lab, ch, cw, H, W), plane, ch, cw, 5, 4, conf)
    _check(_canvas(lab, ch, cw, H, W), plane, ch, cw, 5, 4)


def test_single_pixel_zones_at_every_boundary():
    H, W, ch, cw, chunk = _geom()
    n = ch * cw
    flat = [0, n - 1, chunk - 1, chunk, 2 * chunk - 1, 2 * chunk, 63, 64, 64 * 32 - 1, 64 * 32,
            cw - 1, cw, 5 * cw - 1, 5 * cw, (ch - 1) * cw - 1, (ch - 1) * cw, chunk + 63, chunk + 64]
    assert len(set(flat)) == len(flat) <= 32 and max(flat) < n
    plane = np.zeros(n, np.uint32)
    for k, i in enumerate(flat):
        plane[i] |= np.uint32(1) << np.uint32(k)
    plane = plane.reshape(ch, cw)
    rng = np.random.default_rng(2)
    lab = _blocks(rng, ch, cw, 6)
    (t,) = _check(_canvas(lab, ch, cw, H, W), plane, ch, cw, 1 + len(flat), 6)
    for k, i in enumerate(flat):
        row = t.pixels[1 + k]
        assert row.sum() == 1 and row[lab.reshape(-1)[i]] == 1, (k, i)


def test_only_bit_31():
    H, W, ch, cw, _ = _geom()
    plane = np.zeros((ch, cw), np.uint32)
    plane[3:ch - 5, 2:cw - 1] = 0x80000000
    rng = np.random.default_rng(3)
    lab = _blocks(rng, ch, cw, 21)
    (t,) = _check(_canvas(lab, ch, cw, H, W), plane, ch, cw, 33, 21)
    assert t.pixels[1:32].sum() == 0 and t.pixels[32].sum() == (ch - 8) * (cw - 3)


def test_frame_row_alone_with_a_null_plane():
    H, W, ch, cw, _ = _geom()
    rng = np.random.default_rng(4)
    lab = _blocks(rng, ch, cw, 21)
    conf = rng.integers(0, 256, (1, H, W), dtype=np.uint8)
    (t,) = _check(_canvas(lab, ch, cw, H, W), None, ch, cw, 1, 21, conf)
    assert t.rows == 1 and t.pixels.sum() == ch * cw


def test_256_classes_in_16_rows():
    H, W, ch, cw, _ = _geom()
    i = np.arange(ch * cw)
    lab = ((i * 7 + i // 300) % 256).astype(np.uint8).reshape(ch, cw)
    assert len(np.unique(lab)) == 256
    y, x = np.mgrid[:ch, :cw]
    plane = (((x // 7) * 37 + (y // 5) * 1013) % (1 << 15)).astype(np.uint32)
    assert np.bitwise_or.reduce(plane, axis=None) == (1 << 15) - 1
    rng = np.random.default_rng(5)
    conf = rng.integers(0, 256, (1, H, W), dtype=np.uint8)
    (t,) = _check(_canvas(lab, ch, cw, H, W), plane, ch, cw, 16, 256, conf)
    assert (t.pixels[0] > 0).all()


def test_labels_past_the_classes_count_nowhere():
    H, W, ch, cw, _ = _geom()
    rng = np.random.default_rng(6)
    lab = rng.integers(0, 256, (ch, cw)).astype(np.uint8)
    lab[:, :40] = _blocks(rng, ch, 40, 256, speckle=0.0)
    plane = rng.integers(0, 8, (ch, cw)).astype(np.uint32)
    conf = rng.integers(0, 256, (1, H, W), dtype=np.uint8)
    (t,) = _check(_canvas(lab, ch, cw, H, W), plane, ch, cw, 4, 5, conf)
    assert 0 < t.pixels[0].sum() == int((lab < 5).sum()) < ch * cw


@pytest.mark.parametrize("codes", ["all255", "random", "none"])
def test_confidence_blocks(codes):
    H, W, ch, cw, _ = _geom()
    rng = np.random.default_rng(7)
    lab = _blocks(rng, ch, cw, 21)
    zl = [ZN.Zone("a", ((0.1, 0.1), (0.8, 0.2), (0.5, 0.9))), ZN.Zone("b", ((0.5, 0.0), (1.0, 0.0), (1.0, 1.0), (0.5, 1.0)))]
    plane = ZN.rasterize(zl, cw, ch)
    conf = {"all255": np.full((1, H, W), 255, np.uint8), "none": None,
            "random": rng.integers(0, 256, (1, H, W), dtype=np.uint8)}[codes]
    (t,) = _check(_canvas(lab, ch, cw, H, W), plane, ch, cw, 3, 21, conf)
    if codes == "all255":
        assert np.array_equal(t.sum_conf, 255 * t.pixels)
    if codes == "none":
        assert t.sum_conf is None


def test_three_frames_of_three_kinds_share_one_plane():
    H, W, ch, cw, _ = _geom()
    rng = np.random.default_rng(8)
    y, x = np.mgrid[:ch, :cw]
    kinds = [np.full((ch, cw), 3, np.uint8), (1 + ((x + y) & 1)).astype(np.uint8), _blocks(rng, ch, cw, 9)]
    plane = ZN.rasterize([ZN.Zone("r", ((0.2, 0.3), (0.9, 0.3), (0.9, 0.8), (0.2, 0.8))),
                          ZN.Zone("t", ((0.0, 0.0), (1.0, 0.5), (0.0, 1.0)))], cw, ch)
    conf = rng.integers(0, 256, (3, H, W), dtype=np.uint8)
    for rot in range(3):
        order = [kinds[(rot + k) % 3] for k in range(3)]
        _check(_canvas(np.stack(order), ch, cw, H, W), plane, ch, cw, 3, 9, conf)


@pytest.mark.parametrize("crop", [(1, 1), (1, 200), (200, 1), (9, 63), (9, 64), (9, 65), (5, 255), (5, 256),
                                  (5, 257)])
def test_thin_and_wave_sized_crops(crop):
    ch, cw = crop
    rng = np.random.default_rng(100 * ch + cw)
    lab = _blocks(rng, ch, cw, 7, speckle=0.1)
    plane = rng.integers(0, 4, (ch, cw)).astype(np.uint32)
    conf = rng.integers(0, 256, (2, ch + 3, cw + 4), dtype=np.uint8)
    _check(_canvas(np.stack([lab, lab[::-1, ::-1]]), ch, cw), plane, ch, cw, 3, 7, conf)


def test_seeded_random_cases():
    """200 tiny cases: piecewise-constant labels plus speckle against random rectangles and
    triangles, random R, C, batch and crop, with and without confidence."""
    rng = np.random.default_rng(2024)
    for case in range(200):
        ch, cw = int(rng.integers(1, 40)), int(rng.integers(1, 150))
        Z, C, B = int(rng.integers(0, 6)), int(rng.integers(1, 30)), int(rng.integers(1, 4))
        zl = []
        for k in range(Z):
            p = rng.uniform(-0.2, 1.2, (3, 2))
            if k % 2:
                (x0, y0), (x1, y1) = p[0], p[1]
                p = np.array([[x0, y0], [x1, y0], [x1, y1], [x0, y1]])
            zl.append(ZN.Zone(f"z{k}", tuple(map(tuple, p.tolist()))))
        plane = ZN.rasterize(zl, cw, ch, warn=False) if Z else None
        top = 256 if case % 5 == 0 else C  # some cases hold labels >= C
        lab = np.stack([_blocks(rng, ch, cw, top, speckle=0.05) for _ in range(B)])
        conf = rng.integers(0, 256, (B, ch + 3, cw + 4), dtype=np.uint8) if case % 2 else None
        _check(_canvas(lab, ch, cw), plane, ch, cw, 1 + Z, C, conf)


def _launch_into(lab, plane, cf, out, ws, ch, cw, R, C):
    B, H, W = lab.shape
    _hip().zone_stats(lab, out, ws, B=B, H=H, W=W, crop_h=ch, crop_w=cw, R=R, C=C, plane=plane, conf=cf)


def test_reused_buffers_and_graph_replay_on_new_contents():
    """Two runs on the same buffers with different labels and a different plane, then the same
    inside a captured graph replayed on new contents: nothing of the previous run survives."""
    H, W, ch, cw, _ = _geom()
    rng = np.random.default_rng(9)
    R, C, B = 4, 12, 2

    def contents():
        lab = _canvas(np.stack([_blocks(rng, ch, cw, C) for _ in range(B)]), ch, cw, H, W)
        plane = rng.integers(0, 8, (ch, cw)).astype(np.uint32) * (rng.random((ch, cw)) < 0.5)
        conf = rng.integers(0, 256, (B, H, W), dtype=np.uint8)
        return lab, plane.astype(np.uint32), conf

    out, ws, nb = _buffers(B, R, C, True)
    lab_d = torch.zeros((B, H, W), dtype=torch.uint8, device=DEV)
    cf_d = torch.zeros((B, H, W), dtype=torch.uint8, device=DEV)
    pl_d = torch.zeros((ch, cw), dtype=torch.int32, device=DEV)

    def load(lab, plane, conf):
        lab_d.copy_(torch.from_numpy(lab))
        cf_d.copy_(torch.from_numpy(conf))
        pl_d.copy_(torch.from_numpy(plane.view(np.int32)))

    for _ in range(2):  # eager, twice on the same buffers
        lab, plane, conf = contents()
        load(lab, plane, conf)
        _launch_into(lab_d, pl_d, cf_d, out, ws, ch, cw, R, C)
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy().view(np.uint32), _want(lab, plane, ch, cw, R, C, conf))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g):
            _launch_into(lab_d, pl_d, cf_d, out, ws, ch, cw, R, C)
    torch.cuda.current_stream().wait_stream(s)
    for _ in range(3):
        lab, plane, conf = contents()
        load(lab, plane, conf)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy().view(np.uint32), _want(lab, plane, ch, cw, R, C, conf))
    assert (ws[nb:].cpu().numpy() == WS_SENT).all()


def test_limit_geometry_closed_form():
    """The largest crop, 4096 x 4095 (N < 2^24): one class in all 32 zones with codes 255, so
    pixels = N and sum_conf = 255 N < 2^32 in every row. The expectation is closed-form (the
    numpy definition takes tens of seconds at this size)."""
    ch, cw, R, C, cls = 4095, 4096, 33, 3, 2
    n = ch * cw
    assert n < ZN.MAX_PIXELS and 255 * n < 1 << 32
    lab = torch.full((1, ch, cw), cls, dtype=torch.uint8, device=DEV)
    cf = torch.full((1, ch, cw), 255, dtype=torch.uint8, device=DEV)
    plane = torch.full((ch, cw), -1, dtype=torch.int32, device=DEV)
    out, ws, nb = _buffers(1, R, C, True)
    _launch_into(lab, plane, cf, out, ws, ch, cw, R, C)
    torch.cuda.synchronize()
    want = np.zeros(ZN.frame_words(R, C, True), np.uint32)
    want[:4] = (R, n, cw, ch)
    want[4 + cls:4 + R * C:C] = n
    want[4 + R * C + cls::C] = 255 * n
    assert np.array_equal(out.cpu().numpy().view(np.uint32)[0], want)
    assert (ws[nb:].cpu().numpy() == WS_SENT).all()


def test_wrapper_rejects_bad_arguments_without_launching():
    hip = _hip()
    R, C = 3, 8
    lab = torch.zeros((1, 9, 12), dtype=torch.uint8, device=DEV)
    cf = torch.zeros((1, 9, 12), dtype=torch.uint8, device=DEV)
    plane = torch.zeros((8, 11), dtype=torch.int32, device=DEV)
    out, ws, _ = _buffers(1, R, C, False)
    outc, _, _ = _buffers(1, R, C, True)

    def go(**kw):
        a = dict(lab=lab, out=out, ws=ws, crop_h=8, crop_w=11, R=R, C=C, plane=plane, conf=None, B=1, H=9, W=12)
        a.update(kw)
        hip.zone_stats(a["lab"], a["out"], a["ws"], B=a["B"], H=a["H"], W=a["W"], crop_h=a["crop_h"],
                       crop_w=a["crop_w"], R=a["R"], C=a["C"], plane=a["plane"], conf=a["conf"])

    with pytest.raises(ValueError):
        go(lab=lab.cpu())
    with pytest.raises(TypeError):
        go(lab=lab.to(torch.int32))
    with pytest.raises(ValueError):
        go(lab=torch.zeros((1, 9, 24), dtype=torch.uint8, device=DEV)[:, :, ::2])  # non-contiguous
    with pytest.raises(ValueError):
        go(H=10)  # labels are not [B, H, W]
    with pytest.raises(TypeError):
        go(out=out.float())
    wide = torch.full((1, 2 * (4 + R * C)), SENT, dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError):
        go(out=wide[:, ::2])
    with pytest.raises(ValueError):
        go(out=outc)  # the confidence shape without conf
    with pytest.raises(ValueError):
        go(conf=cf)  # conf with the one-block shape
    with pytest.raises(TypeError):
        go(conf=cf.to(torch.int32), out=outc)
    with pytest.raises(ValueError):
        go(conf=cf[:, :8], out=outc)
    with pytest.raises(ValueError):
        go(crop_h=10)  # crop > map
    with pytest.raises(ValueError):
        go(crop_w=13)
    with pytest.raises(ValueError):
        go(crop_h=0)
    with pytest.raises(ValueError):
        go(plane=None)  # R > 1 needs a plane
    with pytest.raises(ValueError):
        go(R=1, out=torch.full((1, 4 + C), SENT, dtype=torch.int32, device=DEV))  # R == 1 takes none
    with pytest.raises(TypeError):
        go(plane=plane.float())
    with pytest.raises(ValueError):
        go(plane=plane[:7])
    with pytest.raises(ValueError):
        go(plane=plane.cpu())
    with pytest.raises(ValueError):
        go(R=34, out=torch.full((1, 4 + 34 * C), SENT, dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError):
        go(C=257, out=torch.full((1, 4 + R * 257), SENT, dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError):
        go(C=0)
    with pytest.raises(ValueError):  # 17 * 256 = 4352 counters > ZONE_COUNTERS
        go(R=17, C=256, out=torch.full((1, 4 + 17 * 256), SENT, dtype=torch.int32, device=DEV))
    with pytest.raises(TypeError):
        go(ws=ws.to(torch.int32))
    with pytest.raises(ValueError):
        go(ws=ws.cpu())
    with pytest.raises(ValueError):
        go(B=2)
    big = torch.zeros((1, 4096, 4096), dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError):  # N = 2^24
        hip.zone_stats(big, torch.full((1, 4 + C), SENT, dtype=torch.int32, device=DEV), ws, B=1, H=4096,
                       W=4096, crop_h=4096, crop_w=4096, R=1, C=C)
    many = torch.zeros((65536, 1, 1), dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError):
        hip.zone_stats(many, torch.full((65536, 4 + C), SENT, dtype=torch.int32, device=DEV), ws, B=65536,
                       H=1, W=1, crop_h=1, crop_w=1, R=1, C=C)
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == SENT).all() and (outc.cpu().numpy() == SENT).all()
    assert (wide.cpu().numpy() == SENT).all() and (ws.cpu().numpy() == WS_SENT).all()


# ---- engine and pipeline -------------------------------------------------------------------

ZONES = {"zones": [{"name": "left", "rect": [0.0, 0.0, 0.5, 1.0]},
                   {"name": "right", "rect": [0.5, 0.0, 1.0, 1.0]},
                   {"name": "tri", "polygon": [[0.1, 0.1], [0.9, 0.25], [0.4, 0.95]]},
                   {"name": "off", "rect": [1.5, 1.5, 2.0, 2.0]}]}


@pytest.fixture(scope="module")
def zone_file(tmp_path_factory):
    p = tmp_path_factory.mktemp("zones") / "zones.json"
    p.write_text(json.dumps(ZONES))
    return str(p)


def _cfg(**kw):
    from semantic_segmentation_server_amd import config as C
    base = dict(input_size=129, batch=2, backend="hip", graph=False, min_area_ratio=0.0005)
    base.update(kw)
    return C.Config(**base)


def _oracle(eng, frames):
    """The zone words of the engine's own label maps (and confidence planes) of ``frames``."""
    labels, conf = eng._infer(frames.to(DEV))
    torch.cuda.synchronize()
    labels = labels.cpu().numpy()
    conf = conf.cpu().numpy() if conf is not None and eng.zone_conf else None
    return np.stack([ZN.encode(labels[b], eng.zone_plane, eng.crop_w, eng.crop_h, eng.zone_classes,
                               rows=eng.zone_rows, conf=None if conf is None else conf[b])
                     for b in range(len(labels))])


@pytest.mark.parametrize("graph", [False, True])
def test_engine_step_zones_are_those_of_its_labels(graph, zone_file):
    from semantic_segmentation_server_amd.runtime.engine import Engine
    from semantic_segmentation_server_amd.runtime.sources import SyntheticSource
    eng = Engine(_cfg(graph=graph, serve_zones=True, zones=zone_file, serve_confidence=True), torch.device(DEV))
    assert eng.zone_rows == 5 and eng.zone_classes == 21 and eng.zone_conf
    src = SyntheticSource(200, 150, pool=4, seed=7)
    for k in range(2):
        f, _, _ = src.read_batch(2)
        eng.step(f, [2 * k, 2 * k + 1], [1.0, 2.0], [0, 1])
        got = eng.zones.copy()
        assert got.shape == (2, 4 + 2 * 5 * 21) and got.dtype == np.uint32
        want = _oracle(eng, torch.from_numpy(f))
        assert np.array_equal(got, want)
        t = ZN.decode(got[0], conf=True)
        n = eng.crop_w * eng.crop_h
        assert t.pixels[0].sum() == n == t.pixels[1].sum() + t.pixels[2].sum() and t.pixels[4].sum() == 0
        assert 0 < t.pixels[3].sum() < n and t.sum_conf[0].sum() > 0


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


def test_pipeline_pushes_the_latest_zones_and_flag_off_is_the_parent(zone_file):
    from semantic_segmentation_server_amd.runtime.engine import Engine
    from semantic_segmentation_server_amd.runtime.results import ResultHub
    n = 2 * 3 + 1  # 2 * nslots + 1
    batches = _batches(n)
    eng = Engine(_cfg(graph=True, serve_zones=True, zones=zone_file), torch.device(DEV))
    hub = ResultHub(2, maxlen=100000)
    pipe, recs = _drive(eng, batches, hub)
    want = _oracle(eng, batches[-1])
    for s in range(2):
        z = hub.zones(s)
        assert z is not None and not z.conf and z.frame_id == 100 + 2 * (n - 1) + s and z.ts == n + 0.5 * s
        assert np.array_equal(z.words, want[s])
    # flag off: no launch, no buffer, and the records are bit-equal to the run with zones
    off = Engine(_cfg(graph=True), torch.device(DEV))
    hub_off = ResultHub(2, maxlen=100000)
    pipe_off, recs_off = _drive(off, batches, hub_off)
    assert off.zone_rows == 0 and off.zone_packed is None and off.zones is None
    assert pipe_off.local_zones is None and hub_off.zones(0) is None
    post = off._hip_post
    assert post.zone_rows == 0 and not post._zone_bufs and not post._zone_plane and post.last_zones is None
    assert len(recs) > 0 and recs.tobytes() == recs_off.tobytes()


@pytest.mark.parametrize("graph", [False, True])
def test_masks_regions_confidence_tracks_and_zones_together(graph, zone_file):
    from semantic_segmentation_server_amd.postprocess import mask_rle as MR
    from semantic_segmentation_server_amd.postprocess import regions as RG
    from semantic_segmentation_server_amd.postprocess import tracks as TK
    from semantic_segmentation_server_amd.runtime.engine import Engine
    eng = Engine(_cfg(graph=graph, serve_zones=True, zones=zone_file, serve_masks=True, mask_max_runs=4096,
                      serve_regions=True, max_regions=8, serve_confidence=True, track_regions=True,
                      streams=2), torch.device(DEV))
    trk = {s: TK.StreamTracker(eng.track_q) for s in (0, 1)}
    batches = _batches(3)
    for k, f in enumerate(batches):
        eng.step(f.numpy(), [2 * k, 2 * k + 1], [0.0, 0.0], [0, 1])
        zones, regions, masks = eng.zones.copy(), eng.regions.copy(), eng.masks.copy()
        labels, conf = eng._infer(f.to(DEV))
        torch.cuda.synchronize()
        labels, conf = labels.cpu().numpy(), conf.cpu().numpy()
        assert np.array_equal(zones, _oracle(eng, f))
        for b in range(2):
            wr = RG.encode(labels[b], eng.crop_w, eng.crop_h, eng.region_mask, eng.region_min_pixels,
                           eng.region_cap, out=np.zeros(4 + eng.region_words * eng.region_cap, np.uint32),
                           tracker=trk[b], conf=conf[b])
            u = RG.used_words(wr, eng.region_cap, conf=True, tracks=True)
            assert np.array_equal(regions[b, :u], wr[:u]), (k, b)
            wm = MR.encode(labels[b], eng.crop_w, eng.crop_h, eng.mask_cap)
            um = 4 + min(int(wm[0]), eng.mask_cap)
            assert np.array_equal(masks[b, :um], wm[:um]), (k, b)
