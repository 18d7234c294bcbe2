"""Cost of --serve_confidence on the benchmark shape (B = 32, 640 x 480 camera, 33 x 33 x 21
logits -> 513 x 513), on the bench model's own logits and label maps.

    python scripts/confidence_bench.py [--batch 32] [--steps 60] [--warmup 15] [--rounds 3]

Three measurements, one JSON line at the end:

1. the two-plane kernel ``upsample_argmax_conf`` against the label-only ``upsample_argmax``
   variant that assets/tune_mi355x.json picks for this plan shape (what a plan without the
   flag runs), on the logits buffer of the plan;
2. ``class_regions`` with and without ``sum_conf`` on the plan's label maps and confidence
   plane (the device words are checked against postprocess/regions.py first);
3. frames/s of the serving-shaped step loop (bench.py's: slot-parallel graphs, lag 2, records
   and region words to a hub) with --serve_regions against --serve_regions --serve_confidence,
   the two engines alternating over ``rounds`` rounds.

Kernel times come from hipGraph replays of ``reps`` launches (Python launches of a us-scale
kernel measure the host); the two sides of a comparison alternate trial by trial.
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
from semantic_segmentation_server_amd.models.plan import TUNE_FILE_DEFAULT  # noqa: E402
from semantic_segmentation_server_amd.ops import hip_ops  # noqa: E402
from semantic_segmentation_server_amd.postprocess import regions as RG  # noqa: E402


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


def graph_us_ab(fns: dict, reps: int = 50, trials: int = 9) -> dict:
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


def kernels(a, eng, frames) -> dict:
    """Measurements 1 and 2 on the plan buffers of one eager step of ``eng`` (confidence on)."""
    B, Hc, Wc, _ = frames.shape
    eng.set_camera(Wc, Hc)
    eng._step_device(frames)
    torch.cuda.synchronize()
    hm = eng._hip_model
    bufs = hm.buffers(B, Hc, Wc)
    logits, labels, conf = bufs["logits"], bufs["labels"], bufs["conf"]
    _, h, w, ldk = logits.shape
    H, W, K = eng.H, eng.W, hm.num_classes
    key = f"{hm.kind}:B={B}:cam={Wc}x{Hc}:in={H}"
    with open(TUNE_FILE_DEFAULT) as f:
        pick = json.load(f).get(key, {}).get("upsample")
    if pick is None:
        pick = "lane"
        print(f"no saved upsample pick for {key}: comparing against 'lane'")
    lab2, lab3, cf2 = torch.empty_like(labels), torch.empty_like(labels), torch.empty_like(conf)
    shape = dict(B=B, h=h, w=w, K=K, ldk=ldk, H=H, W=W)
    t = graph_us_ab({
        "argmax": lambda: hip_ops.upsample_argmax(logits, lab2, variant=hip_ops.UPSAMPLE_VARIANTS[pick], **shape),
        "argmax_conf": lambda: hip_ops.upsample_argmax_conf(logits, lab3, cf2, **shape)})
    torch.cuda.synchronize()
    agree = (lab2 == lab3).float().mean().item()
    codes = cf2.cpu().numpy()
    print(f"upsample, B = {B}, {h} x {w} x {K} -> {H} x {W}: argmax ({pick}) {t['argmax'][0]:.1f} us min "
          f"{t['argmax'][1]:.1f} us median; argmax + confidence {t['argmax_conf'][0]:.1f} / "
          f"{t['argmax_conf'][1]:.1f} us; labels agree on {agree:.6f} of the pixels; codes min "
          f"{codes.min()} median {int(np.median(codes))} max {codes.max()}")
    out = {"upsample_pick": pick, "argmax_us": round(t["argmax"][1], 1), "argmax_us_min": round(t["argmax"][0], 1),
           "argmax_conf_us": round(t["argmax_conf"][1], 1), "argmax_conf_us_min": round(t["argmax_conf"][0], 1),
           "labels_agree": agree, "exp_per_step": B * H * W * K}

    cw, ch, cap = eng.crop_w, eng.crop_h, eng.region_cap
    cls, mp = eng.region_mask, eng.region_min_pixels
    w6 = torch.zeros((B, 4 + 6 * cap), dtype=torch.int32, device=labels.device)
    w7 = torch.zeros((B, 4 + 7 * cap), dtype=torch.int32, device=labels.device)
    ws6 = torch.zeros(hip_ops.class_regions_workspace_bytes(B, ch, cw), dtype=torch.uint8, device=labels.device)
    ws7 = torch.zeros(hip_ops.class_regions_workspace_bytes(B, ch, cw, True), dtype=torch.uint8,
                      device=labels.device)
    geo = dict(B=B, H=H, W=W, crop_h=ch, crop_w=cw, classes=cls, min_pixels=mp, K=cap)
    fns = {"regions": lambda: hip_ops.class_regions(labels, w6, ws6, **geo),
           "regions_conf": lambda: hip_ops.class_regions(labels, w7, ws7, conf=conf, **geo)}
    for f in fns.values():
        f()
    torch.cuda.synchronize()
    lab_h, conf_h = labels.cpu().numpy(), conf.cpu().numpy()
    g6, g7 = w6.cpu().numpy().view(np.uint32), w7.cpu().numpy().view(np.uint32)
    n = []
    for b in range(B):
        want6 = RG.encode(lab_h[b], cw, ch, cls, mp, cap)
        want7 = RG.encode(lab_h[b], cw, ch, cls, mp, cap, conf=conf_h[b])
        assert np.array_equal(g6[b, :RG.used_words(want6)], want6[:RG.used_words(want6)]), b
        assert np.array_equal(g7[b, :RG.used_words(want7, conf=True)], want7[:RG.used_words(want7, conf=True)]), b
        n.append(int(want7[0]))
    t = graph_us_ab(fns, reps=20)
    print(f"class_regions, B = {B}, crop {cw} x {ch}, {min(n)} .. {max(n)} regions a frame: "
          f"{t['regions'][0]:.1f} us min {t['regions'][1]:.1f} us median; with sum_conf "
          f"{t['regions_conf'][0]:.1f} / {t['regions_conf'][1]:.1f} us (device words equal the definition's)")
    out.update(regions_us=round(t["regions"][1], 1), regions_us_min=round(t["regions"][0], 1),
               regions_conf_us=round(t["regions_conf"][1], 1), regions_conf_us_min=round(t["regions_conf"][0], 1),
               regions_per_frame=[min(n), int(np.median(n)), max(n)])
    return out


def end_to_end(a, engines: dict, batches) -> dict:
    """Measurement 3: frames/s of bench.py's step loop per engine, alternating over rounds."""
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
              f"({a.steps} steps of {a.batch}; region rows of {7 if r.conf else 6} words)")
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
        print("confidence_bench: needs a GPU", file=sys.stderr)
        return 1
    from semantic_segmentation_server_amd.runtime.engine import Engine
    from semantic_segmentation_server_amd.runtime.sources import SyntheticSource
    dev = torch.device("cuda", 0)
    cam_w, cam_h = (int(v) for v in a.camera.split("x"))
    src = SyntheticSource(cam_w, cam_h, stream=0, seed=1, pool=max(2, min(a.batch, 8)))
    batches = [torch.from_numpy(np.ascontiguousarray(src.read_batch(a.batch)[0])).pin_memory() for _ in range(2)]
    engines = {"regions": Engine(_cfg(a), dev), "regions_conf": Engine(_cfg(a, serve_confidence=True), dev)}
    out = kernels(a, engines["regions_conf"], batches[0].to(dev))
    out.update(end_to_end(a, engines, batches))
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
