"""Cost of the class-region kernels (csrc/hip/class_regions.hip) on real and planted label maps.

    python bench.py --gpus 1 --steps 20 --warmup 5 --dump-outputs DIR
    python scripts/regions_bench.py [DIR/labels.npy] [--camera 640x480] [--crop WxH] [--k N]

Two sets of maps: the dumped ones of the bench model (random-init weights: speckled), if given,
and planted piecewise-constant ones (postprocess/synthetic.py: blocks and blobs with a little
noise, like the argmax of trained weights). Per set it prints the region counts (numpy
definition, postprocess/regions.py), checks the device words against it, and times the region
kernels at B = 32 and B = 1 from hipGraph replays (``reps`` launches per graph: Python launches
of a us-scale kernel measure the host). The device post-processing and the mask encoder are
timed on the same maps in the same harness, for scale. One JSON line at the end.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from semantic_segmentation_server_amd.labels import colormap_for  # noqa: E402
from semantic_segmentation_server_amd.ops import hip_ops  # noqa: E402
from semantic_segmentation_server_amd.postprocess import regions as RG  # noqa: E402
from semantic_segmentation_server_amd.postprocess import synthetic  # noqa: E402
from semantic_segmentation_server_amd.postprocess.device import DevicePostprocess  # noqa: E402


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


def measure(name, lab, cw, ch, K, mp, classes, mask_cap, post):
    B, H, W = lab.shape
    dev = torch.device("cuda")
    want = [RG.encode(l, cw, ch, classes, mp, K) for l in lab]
    n = [int(w[0]) for w in want]
    every = [len(RG.region_table(l, cw, ch, classes, 1)) for l in lab[:4]]
    print(f"{name}: {B} maps {H} x {W}, crop {cw} x {ch}, min_pixels {mp}: regions per frame min "
          f"{min(n)} median {int(np.median(n))} max {max(n)} (of any size, first 4 maps: {every})")
    out = {"maps": B, "crop": [cw, ch], "min_pixels": mp, "K": K, "regions_min": min(n),
           "regions_median": int(np.median(n)), "regions_max": max(n), "regions_any_size": every}
    for b in (B, 1):
        d = torch.from_numpy(lab[:b]).to(dev)
        words = torch.zeros((b, 4 + 6 * K), dtype=torch.int32, device=dev)
        ws = torch.zeros(hip_ops.class_regions_workspace_bytes(b, ch, cw), dtype=torch.uint8, device=dev)
        mwords = torch.zeros((b, 4 + mask_cap), dtype=torch.int32, device=dev)
        mws = torch.zeros(max(4, hip_ops.mask_rle_workspace_bytes(b, ch, cw)), dtype=torch.uint8, device=dev)

        def reg():
            hip_ops.class_regions(d, words, ws, B=b, H=H, W=W, crop_h=ch, crop_w=cw, classes=classes,
                                  min_pixels=mp, K=K)

        reg()
        torch.cuda.synchronize()
        got = words.cpu().numpy().view(np.uint32)
        for i in range(b):
            u = RG.used_words(want[i])
            assert np.array_equal(got[i, :u], want[i][:u]), f"{name} frame {i}: device words differ from the spec"
        lo, med = graph_us(reg)
        plo, pmed = graph_us(lambda: post.run(d, cw, ch, 0.05 * H * W))
        mlo, mmed = graph_us(lambda: hip_ops.mask_rle(d, mwords, mws, B=b, H=H, W=W, crop_h=ch,
                                                      crop_w=cw, cap=mask_cap))
        print(f"  B = {b:2d}: class_regions {lo:7.1f} us min {med:7.1f} us median per batch; "
              f"postprocess {plo:7.1f} / {pmed:7.1f} us; mask_rle {mlo:7.1f} / {mmed:7.1f} us")
        out[f"class_regions_us_b{b}"] = round(med, 1)
        out[f"class_regions_us_min_b{b}"] = round(lo, 1)
        out[f"postprocess_us_b{b}"] = round(pmed, 1)
        out[f"mask_rle_us_b{b}"] = round(mmed, 1)
    return out


def main() -> int:
    p = argparse.ArgumentParser()
    p.add_argument("labels", nargs="?", default=None,
                   help="labels.npy of bench.py --dump-outputs ([B, H, W] uint8); without it only planted maps")
    p.add_argument("--camera", default="640x480", help="camera the maps were letterboxed from")
    p.add_argument("--crop", default=None, help="valid region WIDTHxHEIGHT (default: the camera's letterbox)")
    p.add_argument("--k", type=int, default=0, help="region records per frame (0: Config default)")
    p.add_argument("--size", type=int, default=513, help="map size of the planted maps")
    p.add_argument("--batch", type=int, default=32, help="planted maps")
    a = p.parse_args()
    from semantic_segmentation_server_amd.config import Config
    cfg = Config()
    K = a.k or cfg.max_regions
    sets = {}
    if a.labels:
        sets["bench"] = np.ascontiguousarray(np.load(a.labels), np.uint8)
    H = W = sets["bench"].shape[1] if sets else a.size
    rng = np.random.default_rng(0)
    sets["planted"] = np.stack([synthetic.random_label_map(rng, H, W) for _ in range(a.batch)]).astype(np.uint8)
    if a.crop:
        cw, ch = (int(v) for v in a.crop.split("x"))
    else:
        from semantic_segmentation_server_amd.ops import reference_ops as R
        cam_w, cam_h = (int(v) for v in a.camera.split("x"))
        cw, ch = R.letterbox_luts(cam_w, cam_h, W, H)[4:6]
    mp = RG.min_pixels_for(cfg.region_min_area_ratio, H, W)
    classes = RG.default_classes(cfg.num_classes)
    post = DevicePostprocess(torch.device("cuda"), H, W, colormap_for("pascal"), 64, bins=21)
    out = {name: measure(name, lab, cw, ch, K, mp, classes, cfg.mask_max_runs, post)
           for name, lab in sets.items()}
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
