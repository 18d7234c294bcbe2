"""Raw 4:2:2 ingest (--pixel_format yuyv | uyvy), the parts that need no GPU: the torch
definition of the conversion against the host's (csrc/host/v4l2.cpp), the numpy encoder, the
sources, feeder and config plumbing, the packed-row copy of the raw capture mode, and the CPU
engine. Every comparison is exact, except the grey round trip, whose bound is derived there."""
import numpy as np
import pytest
import torch

from semantic_segmentation_server_amd import config as C
from semantic_segmentation_server_amd.ops import reference_ops as R
from semantic_segmentation_server_amd.ops.native import host
from semantic_segmentation_server_amd.runtime.feeder import BatchFeeder
from semantic_segmentation_server_amd.runtime.sources import (FileSource, SyntheticSource, bgr_to_yuv422,
                                                              make_source, probe_resolution)

from raw_ingest_ref import exhaustive_stream, host_bgr


@pytest.mark.parametrize("uyvy", [False, True])
def test_torch_definition_equals_the_host_exhaustively(uyvy):
    s = exhaustive_stream()
    want = host_bgr(s, uyvy)
    got = R.yuv422_to_bgr(torch.from_numpy(s), uyvy)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (4096, 8192, 3)
    assert np.array_equal(got.numpy(), want)


@pytest.mark.parametrize("uyvy", [False, True])
def test_torch_definition_equals_the_host_on_random_frames(uyvy):
    x = np.random.default_rng(1).integers(0, 256, (3, 5, 34, 2), dtype=np.uint8)
    got = R.yuv422_to_bgr(torch.from_numpy(x), uyvy=uyvy)
    assert tuple(got.shape) == (3, 5, 34, 3)
    assert np.array_equal(got.numpy(), host_bgr(x, uyvy))
    with pytest.raises(ValueError):
        R.yuv422_to_bgr(torch.zeros((2, 3, 2), dtype=torch.uint8))  # odd width
    with pytest.raises(ValueError):
        R.yuv422_to_bgr(torch.zeros((2, 4, 2), dtype=torch.int32))


def test_encoder_shape_and_byte_orders():
    img = np.random.default_rng(2).integers(0, 256, (7, 10, 3), dtype=np.uint8)
    yuyv = bgr_to_yuv422(img)
    uyvy = bgr_to_yuv422(img, uyvy=True)
    assert yuyv.shape == (7, 10, 2) and yuyv.dtype == np.uint8
    assert np.array_equal(uyvy, yuyv[..., ::-1])
    assert bgr_to_yuv422(np.stack([img, img])).shape == (2, 7, 10, 2)
    # one pixel pair by hand: BT.601 limited range, chroma from the pair's mean
    pair = np.array([[[255, 0, 0], [0, 0, 255]]], np.uint8)  # blue, red (BGR)
    y_b, y_r = 16 + 24.966, 16 + 65.481
    u = 128 + (112.0 - 37.797) / 2
    v = 128 + (112.0 - 18.214) / 2
    assert bgr_to_yuv422(pair).reshape(-1).tolist() == [round(y_b), round(u), round(y_r), round(v)]
    with pytest.raises(ValueError):
        bgr_to_yuv422(np.zeros((4, 5, 3), np.uint8))


def test_grey_ramp_round_trip_within_one_level():
    g = np.arange(256, dtype=np.uint8)
    img = np.repeat(g[None, :, None], 3, axis=2)  # (1, 256, 3), R = G = B = g
    enc = bgr_to_yuv422(img)
    assert (enc[0, :, 1] == 128).all()  # grey: no chroma
    dec = host().yuv422_to_bgr(enc.reshape(1, -1), False)
    # Y is rounded to nearest: at most 0.5 off, scaled by the decoder's 1.164; the decoder
    # rounds to nearest once more: 0.5. 0.582 + 0.5 < 2, so integers differ by at most 1
    assert np.abs(dec.astype(np.int32) - img).max() <= 1


@pytest.mark.parametrize("seed", [0, 5])
def test_synthetic_source_serves_the_encoded_pool(seed):
    raw = SyntheticSource(200, 150, pixel_format="yuyv", seed=seed)
    bgr = SyntheticSource(200, 150, seed=seed)
    assert raw.pixel_format == "yuyv" and bgr.pixel_format == "bgr"
    assert raw.pool.shape == (len(bgr.pool), 150, 200, 2) and raw.pool.dtype == np.uint8
    assert np.array_equal(raw.pool, bgr_to_yuv422(bgr.pool))
    out = np.zeros((3, 150, 200, 2), np.uint8)
    n, ids, ts = raw.read_batch_into(out)
    assert n == 3 and ids == [0, 1, 2] and np.array_equal(out, raw.pool[:3])
    f, ids, _ = raw.read_batch(2)
    assert f.shape == (2, 150, 200, 2) and ids == [3, 4]
    assert raw.advance(2)[1] == [5, 6]
    assert next(raw).image.shape == (150, 200, 2)
    uy = SyntheticSource(200, 150, pixel_format="uyvy", seed=seed)
    assert np.array_equal(uy.pool, raw.pool[..., ::-1])
    with pytest.raises(ValueError):
        SyntheticSource(201, 150, pixel_format="yuyv")
    with pytest.raises(ValueError):
        SyntheticSource(200, 150, pixel_format="nv12")
    assert make_source("synthetic", width=64, height=48, pixel_format="uyvy").pool.shape[-1] == 2


def test_feeder_ring_takes_its_shape_from_the_sources():
    raw = [SyntheticSource(64, 48, stream=s, pool=2, pixel_format="yuyv") for s in range(2)]
    fd = BatchFeeder(raw, 4, ring=2, pin=False)
    assert fd.pixel_format == "yuyv" and fd.shape == (4, 48, 64, 2)
    assert fd.bufs[0].shape[-1] == 2 and tuple(fd.bufs[1].shape) == (4, 48, 64, 2)
    b = fd._fill(0)
    assert np.array_equal(b.frames.numpy()[:2], raw[0].pool[:2])
    assert np.array_equal(b.frames.numpy()[2:], raw[1].pool[:2])
    assert BatchFeeder([SyntheticSource(64, 48, pool=2)], 4, ring=2, pin=False).bufs[0].shape[-1] == 3
    with pytest.raises(ValueError, match="pixel format"):
        BatchFeeder([raw[0], SyntheticSource(64, 48, stream=1, pool=2)], 4, ring=2, pin=False)
    with pytest.raises(ValueError, match="pixel format"):
        BatchFeeder([raw[0], SyntheticSource(64, 48, stream=1, pool=2, pixel_format="uyvy")], 4,
                    ring=2, pin=False)


def test_file_source_checks_the_stack_against_the_format(tmp_path):
    rng = np.random.default_rng(4)
    p2, p3 = str(tmp_path / "raw.npy"), str(tmp_path / "bgr.npy")
    raw = rng.integers(0, 256, (3, 6, 8, 2), dtype=np.uint8)
    np.save(p2, raw)
    np.save(p3, rng.integers(0, 256, (3, 6, 8, 3), dtype=np.uint8))
    src = FileSource(p2, pixel_format="yuyv")
    assert src.resolution == (8, 6) and src.pixel_format == "yuyv"
    assert np.array_equal(np.stack([f.image for f in src]), raw)
    assert probe_resolution("file", path=p2, pixel_format="yuyv") == (8, 6)
    assert FileSource(p3).resolution == (8, 6)
    with pytest.raises(ValueError):
        FileSource(p3, pixel_format="yuyv")
    with pytest.raises(ValueError):
        FileSource(p2)  # bgr
    with pytest.raises(ValueError):
        make_source("file", path=p2, pixel_format="bgr")


def test_packed_row_copy_honours_the_pitch():
    W, H, pitch, sent = 6, 3, 20, 0xEE
    payload = np.random.default_rng(6).integers(0, 200, (H, 2 * W), dtype=np.uint8)
    buf = np.full((H, pitch), sent, np.uint8)
    buf[:, :2 * W] = payload
    out = host().copy_packed_rows(buf.reshape(-1), pitch, W, H)
    assert out.shape == (H, W, 2) and out.dtype == np.uint8
    assert np.array_equal(out.reshape(H, 2 * W), payload)
    # a buffer that ends with the last row's payload (no trailing padding), and pitch == 2 W
    assert np.array_equal(host().copy_packed_rows(buf.reshape(-1)[:pitch * (H - 1) + 2 * W], pitch, W, H), out)
    assert np.array_equal(host().copy_packed_rows(payload.reshape(-1), 2 * W, W, H), out)
    with pytest.raises(ValueError):
        host().copy_packed_rows(buf.reshape(-1), 2 * W - 1, W, H)
    with pytest.raises(ValueError):
        host().copy_packed_rows(buf.reshape(-1)[:pitch * (H - 1)], pitch, W, H)


def test_raw_capture_mode_arguments():
    with pytest.raises(ValueError):
        host().V4L2Capture("/dev/null", 640, 480, 4, "nv12")
    with pytest.raises(RuntimeError, match="QUERYCAP"):
        host().V4L2Capture("/dev/null", 640, 480, raw_format="yuyv")


def test_config_validation():
    assert C.Config().pixel_format == "bgr" and C.Config().frame_channels == 3
    assert C.Config(pixel_format="uyvy").frame_channels == 2
    assert C.parse(["--pixel_format", "yuyv"]).pixel_format == "yuyv"
    with pytest.raises(ValueError, match="pixel_format"):
        C.Config(pixel_format="nv12")
    with pytest.raises(ValueError, match="camera_width"):
        C.Config(pixel_format="yuyv", camera_width=641)
    with pytest.raises(ValueError, match="scatter"):
        C.Config(pixel_format="uyvy", ingest="scatter")
    with pytest.raises(ValueError, match="scatter"):
        C.Config(pixel_format="yuyv").replace(ingest="scatter")
    C.Config(camera_width=641, ingest="scatter")  # bgr: as before


@pytest.mark.parametrize("fmt", ["yuyv", "uyvy"])
def test_cpu_engine_steps_on_raw_frames(fmt):
    from semantic_segmentation_server_amd.runtime.engine import Engine
    base = dict(device="cpu", input_size=129, batch=2, min_area_ratio=0.0005)
    eng = Engine(C.Config(pixel_format=fmt, **base))
    ref = Engine(C.Config(**base))
    assert (eng.frame_channels, ref.frame_channels) == (2, 3)
    raw, _, _ = SyntheticSource(200, 150, pool=2, seed=7, pixel_format=fmt).read_batch(2)
    bgr = host_bgr(raw, fmt == "uyvy")
    recs = eng.step(raw, [4, 5], [1.0, 2.0], [0, 1])
    want = ref.step(bgr, [4, 5], [1.0, 2.0], [0, 1])
    assert len(want) > 0 and recs.dtype == want.dtype and recs.tobytes() == want.tobytes()
    with torch.no_grad():
        assert torch.equal(eng._infer_eager(torch.from_numpy(raw)), ref._infer_eager(torch.from_numpy(bgr)))
    with pytest.raises(ValueError):
        eng.step(bgr, [4, 5], [1.0, 2.0], [0, 1])  # BGR frames into a raw engine
    with pytest.raises(ValueError):
        ref.step(raw, [4, 5], [1.0, 2.0], [0, 1])
