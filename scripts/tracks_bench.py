"""Cost of --track_regions on the benchmark shape (640 x 480 camera -> 513 x 513, crop 513 x 384),
on the bench model's own label maps.

    python scripts/tracks_bench.py [--batch 32] [--steps 60] [--warmup 15] [--rounds 3]

Two measurements, one JSON line at the end:

1. at B = ``batch`` and B = 1 (one stream: every frame's predecessor is the row before it, the
   first row's the carried state), the class-region chain and, beside it, each of the five
   tracking kernels alone and all five together. The device words are checked against
   postprocess/tracks.py first;
2. frames/s of the serving-shaped step loop (bench.py's: slot-parallel graphs, lag 2, records
   and region words to a hub) with --serve_regions against --serve_regions --track_regions, the
   two engines alternating over ``rounds`` rounds.

Kernel times come from hipGraph replays of ``reps`` launches (Python launches of a us-scale
kernel measure the host); the graphs alternate trial by trial.
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
from semantic_segmentation_server_amd.postprocess import regions as RG  # noqa: E402
from semantic_segmentation_server_amd.postprocess import tracks as TK  # noqa: E402


def _graph(fn, reps):
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
    return g


def graph_us_ab(fns: dict, reps: int = 20, trials: int = 9) -> dict:
    """us per call of every ``fn``, each replayed ``reps`` times from its own hipGraph, the
    graphs alternating trial by trial: {name: (min, median)}."""
    graphs = {n: _graph(f, reps) for n, f in fns.items()}
    t = {n: [] for n in fns}
    for _ in range(trials):
        for n, g in graphs.items():
            st, en = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            st.record()
            g.replay()
            en.record()
            en.synchronize()
            t[n].append(st.elapsed_time(en) * 1e3 / reps)
    return {n: (float(min(v)), float(np.median(v))) for n, v in t.items()}


def _cfg(a, **kw):
    cam_w, cam_h = (int(v) for v in a.camera.split("x"))
    return C.Config(arch="mnv2", input_size=a.input_size, backend="hip", batch=a.batch, graph=True,
                    camera_width=cam_w, camera_height=cam_h, serve_regions=True, **kw)


def kernels(eng, labels: torch.Tensor, B: int) -> dict:
    """Measurement 1 on the first ``B`` of the engine's label maps."""
    dev = labels.device
    lab = labels[:B].contiguous()
    H, W, ch, cw, K = eng.H, eng.W, eng.crop_h, eng.crop_w, eng.region_cap
    mp, classes, q = eng.region_min_pixels, eng.region_mask, TK.quantize(eng.cfg.track_min_overlap)
    rows = torch.zeros((B, 4 + 6 * K), dtype=torch.int32, device=dev)
    out = torch.zeros((B, 4 + 8 * K), dtype=torch.int32, device=dev)
    ws = torch.zeros(hip_ops.class_regions_workspace_bytes(B, ch, cw), dtype=torch.uint8, device=dev)
    tws = torch.zeros(hip_ops.region_tracks_workspace_bytes(B, ch, cw, K), dtype=torch.uint8, device=dev)
    state = torch.zeros(hip_ops.region_tracks_state_bytes(1, ch, cw), dtype=torch.uint8, device=dev)
    tables = hip_ops.region_track_tables([B], dev)

    def regions():
        hip_ops.class_regions(lab, rows, ws, B=B, H=H, W=W, crop_h=ch, crop_w=cw, classes=classes,
                              min_pixels=mp, K=K)

    def tracks(kernels=31):
        hip_ops.region_tracks(rows, out, ws, tws, state, tables, counts=[B], crop_h=ch, crop_w=cw, K=K, q=q,
                              kernels=kernels)

    regions()
    tracks()
    regions()
    tracks()  # a second batch of the same maps: its first row continues the last one's regions
    torch.cuda.synchronize()
    got = out.cpu().numpy().view(np.uint32)
    tr = TK.StreamTracker(q)
    host = lab.cpu().numpy()
    n, aged = [], 0
    for rep in range(2):
        for b in range(B):
            want = RG.encode(host[b], cw, ch, classes, mp, K, tracker=tr)
            if rep:
                u = RG.used_words(want, K, tracks=True)
                assert np.array_equal(got[b, :u], want[:u]), f"B = {B} frame {b}: device words differ from the spec"
                n.append(int(want[0]))
                aged += int((RG.decode(want, tracks=True)["age"] > 1).sum())
    fns = {"regions": regions, "tracks": tracks}
    fns.update({name: (lambda m=m: tracks(m)) for name, m in hip_ops.REGION_TRACK_KERNELS.items()})
    t = graph_us_ab(fns)
    print(f"B = {B:2d}, crop {cw} x {ch}, K = {K}, {min(n)} .. {max(n)} regions a frame, {aged} stored regions "
          f"older than one frame (device words equal the definition's)")
    for name, (lo, med) in t.items():
        print(f"    {name:8s} {med:8.1f} us median {lo:8.1f} us min per batch")
    out = {f"{name}_us_b{B}": round(med, 1) for name, (lo, med) in t.items()}
    out[f"regions_per_frame_b{B}"] = [min(n), int(np.median(n)), max(n)]
    return out


def end_to_end(a, engines: dict, batches) -> dict:
    """Measurement 2: frames/s of bench.py's step loop per engine, alternating over rounds."""
    from semantic_segmentation_server_amd.parallel import dist as D
    from semantic_segmentation_server_amd.parallel.dp import DataParallelPipeline
    from semantic_segmentation_server_amd.runtime.results import ResultHub
    ctx = D.init("gloo", device="cuda")
    cam_w, cam_h = (int(v) for v in a.camera.split("x"))
    pipes = {n: DataParallelPipeline(ctx, e, cam_w, cam_h, a.batch, "local", ResultHub(1, maxlen=4096), 1,
                                     lag=2, gather="host", auto_lag=False) for n, e in engines.items()}

    def run(pipe, n):
        pipe.prefetch(batches[0])
        for k in range(n):
            pipe.step(next_frames=batches[(k + 1) % 2] if k + 1 < n else None)
        pipe.flush()
        torch.cuda.synchronize()

    fps = {n: [] for n in pipes}
    for n, p in pipes.items():
        run(p, a.warmup)
    for _ in range(a.rounds):
        for n, p in pipes.items():
            t0 = time.perf_counter()
            run(p, a.steps)
            fps[n].append(a.steps * a.batch / (time.perf_counter() - t0))
    for n, p in pipes.items():
        r = p.hub.regions(0)
        print(f"end to end, {n}: {', '.join(f'{v:.0f}' for v in fps[n])} frames/s "
              f"({a.steps} steps of {a.batch}; region rows of {8 if r.tracks else 6} words)")
        p.close()
    return {f"fps_{n}": [round(v) for v in vs] for n, vs in fps.items()}


def main() -> int:
    p = argparse.ArgumentParser()
    p.add_argument("--batch", type=int, default=32)
    p.add_argument("--input_size", type=int, default=513)
    p.add_argument("--camera", default="640x480")
    p.add_argument("--steps", type=int, default=60)
    p.add_argument("--warmup", type=int, default=15)
    p.add_argument("--rounds", type=int, default=3)
    a = p.parse_args()
    if not torch.cuda.is_available():
        print("tracks_bench: needs a GPU", file=sys.stderr)
        return 1
    from semantic_segmentation_server_amd.runtime.engine import Engine
    from semantic_segmentation_server_amd.runtime.sources import SyntheticSource
    dev = torch.device("cuda", 0)
    cam_w, cam_h = (int(v) for v in a.camera.split("x"))
    src = SyntheticSource(cam_w, cam_h, stream=0, seed=1, pool=max(2, min(a.batch, 8)))
    batches = [torch.from_numpy(np.ascontiguousarray(src.read_batch(a.batch)[0])).pin_memory() for _ in range(2)]
    engines = {"regions": Engine(_cfg(a), dev), "regions_tracks": Engine(_cfg(a, track_regions=True), dev)}
    eng = engines["regions"]
    eng.set_camera(cam_w, cam_h)
    labels = eng._infer_eager(batches[0].to(dev)).clone()
    torch.cuda.synchronize()
    out = {}
    for B in (a.batch, 1):
        out.update(kernels(eng, labels, B))
    out.update(end_to_end(a, engines, batches))
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
