"""Cost of the zone-occupancy kernel (csrc/hip/zone_stats.hip) on real and planted label maps.

    python bench.py --gpus 1 --steps 20 --warmup 5 --dump-outputs DIR
    python scripts/zones_bench.py [DIR/labels.npy] [--camera 640x480] [--crop WxH]

Sets of maps: the dumped ones of the bench model (random-init weights: speckled), if given;
planted piecewise-constant ones (postprocess/synthetic.py); a checkerboard, the worst case of
the kernel's run aggregation (no two neighbours share a key); and two that take the kernel apart
(labels past the classes; one class everywhere). Per set and per zone set (Z = 0:
the frame row alone; Z = 4 rectangles; Z = 32 overlapping zones), with and without a confidence
plane, it checks the device words against the numpy definition (postprocess/zones.py) and times
the kernel at B = 32 and B = 1 from hipGraph replays (``reps`` launches per graph: Python launches
of a us-scale kernel measure the host). The mask encoder, the sibling single-pass kernel, is timed
on the same maps in the same call: it is the yardstick. One JSON line at the end.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from semantic_segmentation_server_amd.ops import hip_ops  # noqa: E402
from semantic_segmentation_server_amd.postprocess import synthetic  # noqa: E402
from semantic_segmentation_server_amd.postprocess import zones as ZN  # noqa: E402


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


def zone_sets():
    """Z = 4 disjoint rectangles (a 2 x 2 grid of areas) and Z = 32 overlapping zones (rectangles
    and triangles that slide across the frame)."""
    four = [ZN.Zone(f"q{k}", ((x, y), (x + 0.4, y), (x + 0.4, y + 0.4), (x, y + 0.4)))
            for k, (x, y) in enumerate([(0.05, 0.05), (0.55, 0.05), (0.05, 0.55), (0.55, 0.55)])]
    many = []
    for k in range(32):
        x, y = 0.02 * k, 0.015 * k
        if k % 2:
            many.append(ZN.Zone(f"z{k}", ((x, y), (x + 0.5, y + 0.1), (x + 0.2, y + 0.5))))
        else:
            many.append(ZN.Zone(f"z{k}", ((x, y), (x + 0.4, y), (x + 0.4, y + 0.45), (x, y + 0.45))))
    return {"Z0": [], "Z4": four, "Z32": many}


def measure(name, lab, cw, ch, C, mask_cap):
    B, H, W = lab.shape
    dev = torch.device("cuda")
    rng = np.random.default_rng(1)
    conf = rng.integers(0, 256, lab.shape, dtype=np.uint8)
    out = {"maps": B, "crop": [cw, ch], "classes": C}
    print(f"{name}: {B} maps {H} x {W}, crop {cw} x {ch}, {C} classes")
    for b in (B, 1):
        d = torch.from_numpy(lab[:b]).to(dev)
        cf = torch.from_numpy(conf[:b]).to(dev)
        mwords = torch.zeros((b, 4 + mask_cap), dtype=torch.int32, device=dev)
        mws = torch.zeros(max(4, hip_ops.mask_rle_workspace_bytes(b, ch, cw)), dtype=torch.uint8, device=dev)
        mlo, mmed = graph_us(lambda: hip_ops.mask_rle(d, mwords, mws, B=b, H=H, W=W, crop_h=ch,
                                                      crop_w=cw, cap=mask_cap))
        out[f"mask_rle_us_b{b}"] = round(mmed, 1)
        print(f"  B = {b:2d}: mask_rle {mlo:7.1f} us min {mmed:7.1f} us median per batch")
        for zname, zl in zone_sets().items():
            R = 1 + len(zl)
            plane = ZN.rasterize(zl, cw, ch, warn=False) if zl else None
            pl = None if plane is None else torch.from_numpy(plane.view(np.int32)).to(dev)
            for with_conf in (False, True):
                words = torch.zeros((b, ZN.frame_words(R, C, with_conf)), dtype=torch.int32, device=dev)
                ws = torch.zeros(hip_ops.zone_stats_workspace_bytes(b, R, C, with_conf), dtype=torch.uint8,
                                 device=dev)

                def run():
                    hip_ops.zone_stats(d, words, ws, B=b, H=H, W=W, crop_h=ch, crop_w=cw, R=R, C=C,
                                       plane=pl, conf=cf if with_conf else None)

                run()
                torch.cuda.synchronize()
                got = words.cpu().numpy().view(np.uint32)
                for i in range(min(b, 2)):  # the oracle on the first frames (it is the slow part)
                    want = ZN.encode(lab[i], plane, cw, ch, C, rows=R, conf=conf[i] if with_conf else None)
                    assert np.array_equal(got[i], want), f"{name} {zname} frame {i}: device words differ"
                lo, med = graph_us(run)
                key = f"zone_stats_us_{zname}{'_conf' if with_conf else ''}_b{b}"
                out[key] = round(med, 1)
                print(f"           zone_stats {zname:>3}{' +conf' if with_conf else '      '} {lo:7.1f} us min "
                      f"{med:7.1f} us median  ({med / mmed:4.2f} x mask_rle)")
    return out


def main() -> int:
    p = argparse.ArgumentParser()
    p.add_argument("labels", nargs="?", default=None,
                   help="labels.npy of bench.py --dump-outputs ([B, H, W] uint8); without it only planted maps")
    p.add_argument("--camera", default="640x480", help="camera the maps were letterboxed from")
    p.add_argument("--crop", default=None, help="valid region WIDTHxHEIGHT (default: the camera's letterbox)")
    p.add_argument("--size", type=int, default=513, help="map size of the planted maps")
    p.add_argument("--batch", type=int, default=32, help="planted maps")
    a = p.parse_args()
    from semantic_segmentation_server_amd.config import Config
    cfg = Config()
    sets = {}
    if a.labels:
        sets["bench"] = np.ascontiguousarray(np.load(a.labels), np.uint8)
    H = W = sets["bench"].shape[1] if sets else a.size
    rng = np.random.default_rng(0)
    sets["planted"] = np.stack([synthetic.random_label_map(rng, H, W) for _ in range(a.batch)]).astype(np.uint8)
    y, x = np.mgrid[:H, :W]
    sets["checkerboard"] = np.repeat((1 + ((x + y) & 1)).astype(np.uint8)[None], a.batch, 0)
    # two sets that take the kernel apart: labels past the classes (no key: the loads, the LDS
    # zeroing and the flush scan alone) and one class everywhere (one run per 64 pixels with all
    # of its zone bits, and at most R non-zero counters a workgroup to flush)
    sets["no_class"] = np.full((a.batch, H, W), 255, np.uint8)
    sets["one_class"] = np.full((a.batch, H, W), 7, np.uint8)
    if a.crop:
        cw, ch = (int(v) for v in a.crop.split("x"))
    else:
        from semantic_segmentation_server_amd.ops import reference_ops as R
        cam_w, cam_h = (int(v) for v in a.camera.split("x"))
        cw, ch = R.letterbox_luts(cam_w, cam_h, W, H)[4:6]
    out = {name: measure(name, lab, cw, ch, cfg.num_classes, cfg.mask_max_runs) for name, lab in sets.items()}
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
