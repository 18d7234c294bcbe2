"""Cost of the label-stabilisation kernel (csrc/hip/label_stable.hip), alone and at the head of
the post-processing graph.

    python scripts/stable_bench.py [--size 513] [--crop 513x385] [--batch 32]

Maps: planted piecewise-constant ones (postprocess/synthetic.py), one base map per stream, with
about 10 % of the pixels relabelled from frame to frame, and uniform confidence codes. Per number
of streams (1 and 4: the rows of feeder.split_batch) and with and without the confidence planes
it checks one out-of-place run against the numpy definition (postprocess/stable.py), outputs and
state words, and times the in-place form -- the one the engine uses -- from hipGraph replays
(``reps`` launches per graph: Python launches of a us-scale kernel measure the host). The bytes
the kernel must move are 2 B in and 2 B out per pixel and frame (half without confidence) plus
8 B of state per stream and crop pixel, once per batch; in place only the crop is touched. Then
the post-processing graph of DevicePostprocess (records, masks, regions with confidence) is timed
with and without the stabilisation in front. One JSON line at the end.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from semantic_segmentation_server_amd.ops import hip_ops  # noqa: E402
from semantic_segmentation_server_amd.postprocess import regions as RG  # noqa: E402
from semantic_segmentation_server_amd.postprocess import stable as SB  # noqa: E402
from semantic_segmentation_server_amd.postprocess import synthetic  # noqa: E402
from semantic_segmentation_server_amd.runtime.feeder import split_batch  # noqa: E402


def graph_us(fn, reps: int = 20, trials: int = 9):
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


def maps(B: int, S: int, H: int, W: int, seed: int = 0):
    """([B, H, W] labels, codes) laid out by split_batch(B, S): per stream one planted map whose
    pixels are relabelled with probability 0.1 in every frame."""
    rng = np.random.default_rng(seed)
    labs = []
    for n in split_batch(B, S):
        base = synthetic.random_label_map(rng, H, W)
        for _ in range(n):
            flip = rng.random((H, W)) < 0.1
            labs.append(np.where(flip, rng.integers(0, 21, (H, W)).astype(np.uint8), base))
    return np.stack(labs).astype(np.uint8), rng.integers(0, 256, (B, H, W)).astype(np.uint8)


def kernel(B, S, H, W, ch, cw, conf, N=3, g=128):
    dev = torch.device("cuda")
    counts = split_batch(B, S)
    lab, code = maps(B, S, H, W)
    g = g if conf else 0
    li = torch.from_numpy(lab).to(dev)
    ci = torch.from_numpy(code).to(dev) if conf else None
    lo, co = torch.empty_like(li), (torch.empty_like(li) if conf else None)
    state = torch.zeros(hip_ops.label_stable_state_bytes(S, ch, cw), dtype=torch.uint8, device=dev)
    tables = hip_ops.label_stable_tables(counts, dev)
    kw = dict(counts=counts, B=B, H=H, W=W, crop_h=ch, crop_w=cw, N=N, g=g)
    hip_ops.label_stable(li, lo, ci, co, state, tables, **kw)
    torch.cuda.synchronize()
    ora = SB.Stabilizers(N, g)
    wl, wc = ora.step(lab, code if conf else None, cw, ch, [s for s, n in enumerate(counts) for _ in range(n)])
    assert np.array_equal(lo.cpu().numpy(), wl), "label_stable: labels differ from the definition"
    assert not conf or np.array_equal(co.cpu().numpy(), wc), "label_stable: codes differ"
    words = state.cpu().numpy().view(np.uint32).reshape(S, -1)
    for s in range(S):
        assert words[s, 0] == 1 and np.array_equal(words[s, 1:], ora.of(s).state_words()), "state differs"
    lo_us, med = graph_us(lambda: hip_ops.label_stable(li, li, ci, ci, state, tables, **kw))
    per_px = 4 if conf else 2
    crop_bytes = B * per_px * ch * cw + 8 * S * ch * cw
    plane_bytes = B * per_px * H * W + 8 * S * ch * cw
    r = {"us_min": round(lo_us, 1), "us_median": round(med, 1), "crop_bytes": crop_bytes,
         "plane_bytes": plane_bytes, "crop_GBps": round(crop_bytes / med / 1e3, 1),
         "plane_GBps": round(plane_bytes / med / 1e3, 1)}
    print(f"label_stable B = {B} S = {S}{' +conf' if conf else '      '}: {lo_us:7.1f} us min {med:7.1f} us "
          f"median; {crop_bytes / 1e6:5.1f} MB of crop and state -> {r['crop_GBps']:7.1f} GB/s "
          f"({plane_bytes / 1e6:5.1f} MB by whole planes -> {r['plane_GBps']:7.1f} GB/s)")
    return r


def post_graph(B, S, H, W, ch, cw, stable: bool):
    from semantic_segmentation_server_amd.config import Config
    from semantic_segmentation_server_amd.labels import colormap_for
    from semantic_segmentation_server_amd.postprocess.device import DevicePostprocess
    cfg = Config()
    dev = torch.device("cuda")
    dp = DevicePostprocess(dev, H, W, np.ascontiguousarray(colormap_for(cfg.dataset), np.int32), cfg.max_segments,
                           bins=cfg.num_classes, mask_cap=cfg.mask_max_runs, region_cap=cfg.max_regions,
                           region_classes=RG.default_classes(cfg.num_classes),
                           region_min_pixels=RG.min_pixels_for(cfg.region_min_area_ratio, H, W),
                           region_conf=True, stable_frames=3 if stable else 0,
                           stable_gate=128 if stable else 0, stable_streams=S if stable else 0)
    lab, code = maps(B, S, H, W)
    li, ci = torch.from_numpy(lab).to(dev), torch.from_numpy(code).to(dev)
    # in place: after the first replay the planes hold the stabilised maps, a fixed point, so both
    # graphs post-process the same kind of map and the difference is the launch in front
    return graph_us(lambda: dp.run(li, cw, ch, cfg.min_area, conf=ci), reps=5)


def main() -> int:
    p = argparse.ArgumentParser()
    p.add_argument("--size", type=int, default=513, help="map size")
    p.add_argument("--crop", default="513x385", help="valid region WIDTHxHEIGHT")
    p.add_argument("--batch", type=int, default=32)
    a = p.parse_args()
    H = W = a.size
    cw, ch = (int(v) for v in a.crop.split("x"))
    out = {"size": a.size, "crop": [cw, ch], "batch": a.batch}
    for S in (1, 4):
        for conf in (False, True):
            out[f"kernel_s{S}{'_conf' if conf else ''}"] = kernel(a.batch, S, H, W, ch, cw, conf)
    for S in (1, 4):
        off_lo, off = post_graph(a.batch, S, H, W, ch, cw, False)
        on_lo, on = post_graph(a.batch, S, H, W, ch, cw, True)
        out[f"post_graph_s{S}"] = {"off_us": round(off, 1), "on_us": round(on, 1), "delta_us": round(on - off, 1)}
        print(f"post graph B = {a.batch} S = {S}: {off:8.1f} us without, {on:8.1f} us with the stabilisation "
              f"(median; min {off_lo:.1f} / {on_lo:.1f}): {on - off:+.1f} us")
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
