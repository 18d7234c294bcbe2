"""Cost of raw 4:2:2 ingest (--pixel_format yuyv): the conversion kernel, the pipeline, the host.

    python scripts/ingest_bench.py [--camera 640x480] [--runs 3] [--out FILE]

1. Kernel: csrc/hip/yuv422.hip at B = 32 and B = 1, timed from hipGraph replays (``reps``
   launches per graph: Python launches of a us-scale kernel measure the host), next to
   ``tensor.copy_`` of a uint8 tensor of B * H * W * 5 / 2 bytes timed the same way -- the
   same bytes read plus written (2 in + 3 out per pixel), the yardstick of a memory-bound
   kernel. The device bytes are checked against the host conversion first.
2. Pipeline: ``DataParallelPipeline`` frames/s at B = 32 and B = 1 fed from two pinned host
   batches, as bench.py feeds it, for ``bgr`` and for ``yuyv``; every run is a fresh process
   and the runs of the two formats alternate, so the table shows the run-to-run spread next
   to the difference.
3. Host: ``host().yuv422_to_bgr`` per frame on this machine (the CPU cost the raw path removes
   from the feeder thread).

One line per measurement, one JSON line at the end; ``--out`` also writes them to a file.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from semantic_segmentation_server_amd import config as C  # noqa: E402
from semantic_segmentation_server_amd.ops import hip_ops  # noqa: E402
from semantic_segmentation_server_amd.ops.native import host  # noqa: E402
from semantic_segmentation_server_amd.runtime.sources import SyntheticSource  # noqa: E402

LINES = []


def say(line: str) -> None:
    print(line, flush=True)
    LINES.append(line)


def graph_us(fn, reps: int = 50, trials: int = 7):
    """us per call of ``fn`` replayed ``reps`` times from one hipGraph: (min, median)."""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            fn()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(reps):
            fn()
    g.replay()
    torch.cuda.synchronize()
    t = []
    for _ in range(trials):
        st, en = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        st.record()
        g.replay()
        en.record()
        en.synchronize()
        t.append(st.elapsed_time(en) * 1e3 / reps)
    return float(min(t)), float(np.median(t))


def kernel_section(out: dict, cam_w: int, cam_h: int) -> None:
    dev = torch.device("cuda")
    pool = SyntheticSource(cam_w, cam_h, seed=1, pool=8, pixel_format="yuyv").pool
    for b in (32, 1):
        raw = pool[np.arange(b) % len(pool)]
        src = torch.from_numpy(raw).to(dev)
        dst = torch.empty((b, cam_h, cam_w, 3), dtype=torch.uint8, device=dev)
        hip_ops.yuv422_to_bgr(src, dst)
        torch.cuda.synchronize()
        want = np.stack([host().yuv422_to_bgr(f.reshape(cam_h, 2 * cam_w), False) for f in raw])
        assert np.array_equal(dst.cpu().numpy(), want), "device conversion differs from the host's"
        nbytes = b * cam_h * cam_w * 5
        ca = torch.zeros(nbytes // 2, dtype=torch.uint8, device=dev)
        cb = torch.empty_like(ca)
        klo, kmed = graph_us(lambda: hip_ops.yuv422_to_bgr(src, dst))
        clo, cmed = graph_us(lambda: cb.copy_(ca))
        say(f"kernel B = {b:2d}: yuv422_to_bgr {klo:7.2f} us min {kmed:7.2f} us median "
            f"({nbytes / kmed / 1e6:6.2f} TB/s); copy_ of {nbytes // 2} B {clo:7.2f} / {cmed:7.2f} us "
            f"({nbytes / cmed / 1e6:6.2f} TB/s); kernel / copy {kmed / cmed:5.2f}")
        out[f"yuv422_us_b{b}"] = round(kmed, 2)
        out[f"yuv422_us_min_b{b}"] = round(klo, 2)
        out[f"copy_us_b{b}"] = round(cmed, 2)
        out[f"copy_us_min_b{b}"] = round(clo, 2)
        out[f"bytes_moved_b{b}"] = nbytes


def pipeline_run(fmt: str, b: int, cam_w: int, cam_h: int, n: int) -> float:
    """frames/s of one timed run of ``n`` steps (after a warm-up) of a fresh pipeline."""
    from semantic_segmentation_server_amd.parallel import dist as D
    from semantic_segmentation_server_amd.parallel.dp import DataParallelPipeline
    from semantic_segmentation_server_amd.runtime.engine import Engine
    ctx = D.init("gloo", device="cuda")
    cfg = C.Config(batch=b, camera_width=cam_w, camera_height=cam_h, pixel_format=fmt)
    src = SyntheticSource(cam_w, cam_h, seed=1, pool=max(2, min(b, 8)), pixel_format=fmt)
    hb = [torch.from_numpy(np.ascontiguousarray(src.read_batch(b)[0])).pin_memory() for _ in range(2)]
    pipe = DataParallelPipeline(ctx, Engine(cfg, ctx.device), cam_w, cam_h, b, "local", None, 1,
                                lag=2, auto_lag=False)

    def run(n: int) -> float:
        pipe.prefetch(hb[0])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for k in range(n):
            pipe.step(next_frames=hb[(k + 1) % 2] if k + 1 < n else None)
        pipe.flush()
        torch.cuda.synchronize()
        return n * b / (time.perf_counter() - t0)

    run(max(20, n // 5))  # warm-up
    return run(n)


def pipeline_section(out: dict, cam_w: int, cam_h: int, runs: int, steps: dict) -> None:
    """Every run is a process of its own (this script with --pipeline-run), the two formats
    alternating. Two engines in one process share its hardware queues: built second in one
    process, the yuyv pipeline measured 38 % below the bgr one at B = 1 (3.76k vs 6.05k
    frames/s); each in a process of its own, 2 % above it ("Raw 4:2:2 ingest")."""
    import subprocess
    for b in (32, 1):
        fps = {"bgr": [], "yuyv": []}
        for _ in range(runs):
            for fmt in fps:
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--camera", f"{cam_w}x{cam_h}",
                                    "--pipeline-run", fmt, str(b), str(steps[b])],
                                   stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
                if r.returncode != 0:
                    raise RuntimeError(f"pipeline run {fmt} B = {b} failed ({r.returncode}):\n{r.stderr[-2000:]}")
                fps[fmt].append(float(r.stdout.strip().splitlines()[-1]))
        for fmt, v in fps.items():
            mb = b * cam_h * cam_w * (3 if fmt == "bgr" else 2) / 1e6
            say(f"pipeline B = {b:2d} {fmt:4s}: " + " ".join(f"{x:8.0f}" for x in v) +
                f" frames/s (median {np.median(v):8.0f}; {steps[b]} steps per run, {mb:.2f} MB per upload)")
            out[f"pipeline_fps_b{b}_{fmt}"] = [round(x) for x in v]
        out[f"pipeline_yuyv_over_bgr_b{b}"] = round(float(np.median(fps["yuyv"]) / np.median(fps["bgr"])), 4)


def host_section(out: dict, cam_w: int, cam_h: int) -> None:
    frame = SyntheticSource(cam_w, cam_h, seed=1, pool=1, pixel_format="yuyv").pool[0].reshape(cam_h, 2 * cam_w)
    f = host().yuv422_to_bgr
    for _ in range(5):
        f(frame, False)
    t = []
    for _ in range(7):
        t0 = time.perf_counter()
        for _ in range(50):
            f(frame, False)
        t.append((time.perf_counter() - t0) / 50 * 1e3)
    say(f"host yuv422_to_bgr {cam_w} x {cam_h}: {min(t):.3f} ms min {np.median(t):.3f} ms median per frame "
        f"(one thread, with the output allocation): {1e3 / np.median(t):.0f} frames/s per converting thread")
    out["host_ms_per_frame"] = round(float(np.median(t)), 3)


def main() -> int:
    p = argparse.ArgumentParser()
    p.add_argument("--camera", default="640x480")
    p.add_argument("--runs", type=int, default=3, help="pipeline runs per format (alternating)")
    p.add_argument("--steps32", type=int, default=600, help="steps per pipeline run at B = 32")
    p.add_argument("--steps1", type=int, default=3000, help="steps per pipeline run at B = 1")
    p.add_argument("--skip-pipeline", action="store_true")
    p.add_argument("--pipeline-run", nargs=3, metavar=("FORMAT", "B", "STEPS"), default=None,
                   help="one timed pipeline run in this process; prints its frames/s (used by the script itself)")
    p.add_argument("--out", default=None, help="also write the printed lines to this file")
    a = p.parse_args()
    if not torch.cuda.is_available():
        print("ingest_bench: needs a GPU", file=sys.stderr)
        return 2
    cam_w, cam_h = (int(v) for v in a.camera.split("x"))
    if a.pipeline_run:
        fmt, b, n = a.pipeline_run[0], int(a.pipeline_run[1]), int(a.pipeline_run[2])
        print(pipeline_run(fmt, b, cam_w, cam_h, n), flush=True)
        return 0
    out = {"camera": [cam_w, cam_h]}
    try:
        host_section(out, cam_w, cam_h)
        if not a.skip_pipeline:  # before this process opens the GPU itself
            pipeline_section(out, cam_w, cam_h, max(3, a.runs), {32: a.steps32, 1: a.steps1})
        kernel_section(out, cam_w, cam_h)
        out["device"] = torch.cuda.get_device_name(0)
        say(json.dumps(out))
    finally:
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as fh:
                fh.write("\n".join(LINES) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
