"""Cost of the label-smoothing kernel (csrc/hip/label_smooth.hip), alone, with its copy back, and
at the head of the post-processing graph; and what the filter does to run and region counts.

    python bench.py --gpus 1 --steps 20 --warmup 5 --dump-outputs DIR
    python scripts/smooth_bench.py [--labels DIR/labels.npy] [--size 513] [--crop 513x385] [--batch 32]

Maps: planted piecewise-constant ones (postprocess/synthetic.py) with 7 % of the pixels replaced
by random labels (seeded), and, with ``--labels``, the dumped maps of the bench model. Per kind
of map, R = 1, 2, 3, B = batch and 1, with and without the confidence planes, it checks the first
frames of one run against the numpy definition (postprocess/smooth.py) and times the launch, and
the launch plus the device-to-device copy back, from hipGraph replays (``reps`` launches per
graph: Python launches of a us-scale kernel measure the host). The traffic floor is 2 B per pixel
for the kernel (1 in, 1 out; twice that with confidence) and as much again for the copy back. The
shares of the kernel's three paths (uniform tile, majority window, counting) are computed on the
host from the same frames. Then the post-processing graph of DevicePostprocess (records, masks,
regions with confidence) is timed with and without the filter in front (R = 1 and 3),
alternating; every replayed chain of either arm first reloads the speckled planes from pristine
copies, because with the filter on ``run`` leaves the smoothed maps in the planes it was given.
The copy back of the kernel timing goes to planes of its own for the same reason. One JSON line
at the end.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from semantic_segmentation_server_amd.ops import hip_ops  # noqa: E402
from semantic_segmentation_server_amd.postprocess import mask_rle as MR  # noqa: E402
from semantic_segmentation_server_amd.postprocess import regions as RG  # noqa: E402
from semantic_segmentation_server_amd.postprocess import smooth as SM  # noqa: E402
from semantic_segmentation_server_amd.postprocess import synthetic  # noqa: E402

HBM_PEAK = 8.0e12  # B/s (spec); about 6.3e12 achievable
CHECKED = 2        # frames of a batch held to the numpy definition


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


def planted(B: int, H: int, W: int, seed: int = 0, share: float = 0.07):
    """[B, H, W] planted piecewise-constant maps with ``share`` of the pixels replaced by random
    labels 0 .. 20, and uniform codes."""
    rng = np.random.default_rng(seed)
    labs = []
    for _ in range(B):
        base = synthetic.random_label_map(rng, H, W)
        hit = rng.random((H, W)) < share
        labs.append(np.where(hit, rng.integers(0, 21, (H, W)).astype(np.uint8), base))
    return np.stack(labs).astype(np.uint8), rng.integers(0, 256, (B, H, W)).astype(np.uint8)


def path_shares(lab, cw, ch, R):
    """Shares of the kernel's paths on ``lab`` [n, H, W]: (tiles copied through as uniform, of
    the tiles with crop pixels; pixels of the other tiles kept by the majority-window test;
    pixels that walk the labels of their window), the last two of all crop pixels."""
    tw, th = hip_ops.label_smooth_tile()
    L = lab[:, :ch, :cw]
    ys, xs = np.arange(ch)[:, None], np.arange(cw)[None, :]
    y0, y1 = np.maximum(ys - R, 0), np.minimum(ys + R + 1, ch)
    x0, x1 = np.maximum(xs - R, 0), np.minimum(xs + R + 1, cw)
    own = np.zeros(L.shape, np.int32)
    for c in np.unique(L):
        I = np.zeros((L.shape[0], ch + 1, cw + 1), np.int32)
        I[:, 1:, 1:] = np.cumsum(np.cumsum(L == c, axis=1, dtype=np.int32), axis=2)
        v = I[:, y1, x1] - I[:, y0, x1] - I[:, y1, x0] + I[:, y0, x0]
        own = np.where(L == c, v, own)
    major = 2 * own >= ((y1 - y0) * (x1 - x0))[None]
    tiles = uni = 0
    in_mixed = np.zeros(L.shape, bool)
    for ty in range(0, ch, th):
        for tx in range(0, cw, tw):
            st = L[:, max(ty - R, 0):ty + th + R, max(tx - R, 0):tx + tw + R]
            u = (st == st[:, :1, :1]).all(axis=(1, 2))
            tiles += len(u)
            uni += int(u.sum())
            in_mixed[:, ty:ty + th, tx:tx + tw] = ~u[:, None, None]
    n = L.size
    return uni / tiles, float((in_mixed & major).sum()) / n, float((in_mixed & ~major).sum()) / n


def counts(lab, cw, ch, classes):
    """(median runs, median regions of the served classes, of any size) per frame of ``lab``."""
    runs = [int(MR.encode(l, cw, ch, 2)[0]) for l in lab]
    regs = [len(RG.table_and_roots(l, cw, ch, classes, 1, None)[0]) for l in lab]
    return int(np.median(runs)), int(np.median(regs))


def kernel(name, lab, code, cw, ch, R, conf):
    dev = torch.device("cuda")
    B, H, W = lab.shape
    li = torch.from_numpy(lab).to(dev)
    ci = torch.from_numpy(code).to(dev) if conf else None
    lo, co = torch.empty_like(li), (torch.empty_like(li) if conf else None)
    kw = dict(B=B, H=H, W=W, crop_h=ch, crop_w=cw, R=R)
    hip_ops.label_smooth(li, lo, ci, co, **kw)
    torch.cuda.synchronize()
    n = min(B, CHECKED)
    wl, wc = SM.apply(lab[:n], code[:n] if conf else None, cw, ch, R)
    assert np.array_equal(lo[:n].cpu().numpy(), wl), "label_smooth: labels differ from the definition"
    assert not conf or np.array_equal(co[:n].cpu().numpy(), wc), "label_smooth: codes differ"
    k_lo, k_med = graph_us(lambda: hip_ops.label_smooth(li, lo, ci, co, **kw))

    back, cback = torch.empty_like(li), (torch.empty_like(li) if conf else None)

    def with_copy():  # the input stays the speckled map: the copy back goes to planes of its own
        hip_ops.label_smooth(li, lo, ci, co, **kw)
        back.copy_(lo)
        if conf:
            cback.copy_(co)

    c_lo, c_med = graph_us(with_copy)
    nbytes = B * H * W * (4 if conf else 2)
    floor_us = nbytes / HBM_PEAK * 1e6
    r = {"us_min": round(k_lo, 1), "us_median": round(k_med, 1), "with_copy_us_median": round(c_med, 1),
         "floor_us": round(floor_us, 2), "GBps": round(nbytes / k_med / 1e3, 1)}
    print(f"label_smooth {name} R = {R} B = {B:2d}{' +conf' if conf else '      '}: {k_lo:7.1f} us min "
          f"{k_med:7.1f} us median ({nbytes / 1e6:5.1f} MB, floor {floor_us:5.2f} us, {r['GBps']:7.1f} GB/s); "
          f"with the copy back {c_med:7.1f} us (floor {2 * floor_us:5.2f} us)")
    return r


def post_graphs(lab, code, cw, ch, R):
    """(off, on, reload) median us of the post-processing chain of DevicePostprocess without and
    with the filter in front, timed alternately, three rounds. With the filter on, ``run`` leaves
    the smoothed maps in the planes it was given, so in both arms every replayed chain first
    reloads the planes from pristine device copies: both process the speckled maps every time.
    ``reload`` is the time of those two copies alone, which both arms contain."""
    from semantic_segmentation_server_amd.config import Config
    from semantic_segmentation_server_amd.labels import colormap_for
    from semantic_segmentation_server_amd.postprocess.device import DevicePostprocess
    cfg = Config()
    dev = torch.device("cuda")
    B, H, W = lab.shape
    times = {0: [], R: []}
    l0, c0 = torch.from_numpy(lab).to(dev), torch.from_numpy(code).to(dev)
    li, ci = torch.empty_like(l0), torch.empty_like(c0)

    def reload():
        li.copy_(l0)
        ci.copy_(c0)

    for _ in range(3):
        for r in (0, R):
            dp = DevicePostprocess(dev, H, W, np.ascontiguousarray(colormap_for(cfg.dataset), np.int32),
                                   cfg.max_segments, bins=cfg.num_classes, mask_cap=cfg.mask_max_runs,
                                   region_cap=cfg.max_regions, region_classes=RG.default_classes(cfg.num_classes),
                                   region_min_pixels=RG.min_pixels_for(cfg.region_min_area_ratio, H, W),
                                   region_conf=True, smooth_radius=r)

            def chain():
                reload()
                dp.run(li, cw, ch, cfg.min_area, conf=ci)

            times[r].append(graph_us(chain, reps=5)[1])
    return float(np.median(times[0])), float(np.median(times[R])), graph_us(reload, reps=5)[1], times


def main() -> int:
    p = argparse.ArgumentParser()
    p.add_argument("--labels", default=None, help="labels.npy of bench.py --dump-outputs ([B, H, W] uint8)")
    p.add_argument("--size", type=int, default=513, help="map size of the planted maps")
    p.add_argument("--crop", default="513x385", help="valid region WIDTHxHEIGHT")
    p.add_argument("--batch", type=int, default=32)
    a = p.parse_args()
    cw, ch = (int(v) for v in a.crop.split("x"))
    kinds = {"planted": planted(a.batch, a.size, a.size)}
    if a.labels:
        lab = np.ascontiguousarray(np.load(a.labels), np.uint8)[:a.batch]
        kinds["dumped"] = (lab, np.random.default_rng(1).integers(0, 256, lab.shape).astype(np.uint8))
    from semantic_segmentation_server_amd.config import Config
    classes = RG.default_classes(Config().num_classes)
    out = {"crop": [cw, ch], "batch": a.batch}
    for name, (lab, code) in kinds.items():
        n = min(len(lab), CHECKED)
        runs, regs = counts(lab[:n], cw, ch, classes)
        print(f"{name}: {len(lab)} maps {lab.shape[1]} x {lab.shape[2]}, crop {cw} x {ch}; unfiltered: "
              f"{runs} runs, {regs} regions per frame (median of {n})")
        out[name] = {"runs": runs, "regions": regs}
        for R in (1, 2, 3):
            sm, _ = SM.apply(lab[:n], None, cw, ch, R)
            runs, regs = counts(sm, cw, ch, classes)
            uni, major, walk = path_shares(lab[:n], cw, ch, R)
            changed = float((sm != lab[:n]).mean())
            print(f"{name} R = {R}: {runs} runs, {regs} regions per frame; {changed:.4f} of the pixels "
                  f"changed; uniform tiles {uni:.3f}, majority-window pixels {major:.3f}, counting "
                  f"pixels {walk:.3f}")
            out[name][f"r{R}"] = {"runs": runs, "regions": regs, "changed": round(changed, 5),
                                  "uniform_tiles": round(uni, 3), "majority_pixels": round(major, 3),
                                  "counting_pixels": round(walk, 3)}
            for b in (len(lab), 1):
                for conf in (False, True):
                    out[name][f"r{R}"][f"b{b}{'_conf' if conf else ''}"] = kernel(
                        name, lab[:b], code[:b], cw, ch, R, conf)
        for R in (1, 3):
            off, on, rel, raw = post_graphs(lab, code, cw, ch, R)
            out[name][f"post_graph_r{R}"] = {"off_us": round(off, 1), "on_us": round(on, 1),
                                             "delta_us": round(on - off, 1), "reload_us": round(rel, 1)}
            print(f"{name}: post graph B = {len(lab)}: {off:8.1f} us without, {on:8.1f} us with the filter "
                  f"(R = {R}; medians of 3 alternating rounds: {[round(v, 1) for v in raw[0]]} / "
                  f"{[round(v, 1) for v in raw[R]]}; both reload the speckled planes first, {rel:.1f} us "
                  f"alone): {on - off:+.1f} us")
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
