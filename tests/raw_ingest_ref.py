"""Shared by the raw-ingest tests (test_raw_ingest_cpu.py, test_raw_ingest_gpu.py): the
exhaustive macropixel stream and the host conversion (csrc/host/v4l2.cpp) of whole batches."""
import numpy as np

from semantic_segmentation_server_amd.ops.native import host


def exhaustive_stream() -> np.ndarray:
    """(4096, 8192, 2): 2^24 macropixels (y0, u, y0 ^ 0x80, v) over every y0, u, v -- every
    (y, u, v) triple in both pixel positions (read as UYVY: every (u, y, v) likewise)."""
    a = np.arange(256, dtype=np.uint8)
    y0, u, v = np.meshgrid(a, a, a, indexing="ij")
    return np.stack([y0, u, y0 ^ 0x80, v], -1).reshape(4096, 8192, 2)


def host_bgr(frames: np.ndarray, uyvy: bool) -> np.ndarray:
    """The host conversion of (..., H, W, 2) packed frames -> (..., H, W, 3)."""
    H, W = frames.shape[-3:-1]
    flat = np.ascontiguousarray(frames).reshape(-1, H, 2 * W)
    return np.stack([host().yuv422_to_bgr(f, uyvy) for f in flat]).reshape(frames.shape[:-1] + (3,))
