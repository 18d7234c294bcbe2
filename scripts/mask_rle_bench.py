"""Cost of the label-mask run-length encoder (csrc/hip/mask_rle.hip) on real label maps.

    python bench.py --gpus 1 --steps 20 --warmup 5 --dump-outputs DIR
    python scripts/mask_rle_bench.py DIR/labels.npy [--camera 640x480] [--crop WxH] [--cap N]

Prints the run counts of the dumped maps (numpy definition, postprocess/mask_rle.py), checks
the device words against it, and times the encoder at B = 32 and B = 1 from hipGraph replays
(``reps`` launches per graph, as the plan autotuner times its variants: Python launches of a
us-scale kernel measure the host). The device post-processing of the same maps is timed the
same way, for scale. One JSON line at the end.
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
from semantic_segmentation_server_amd.postprocess import mask_rle as MR  # noqa: E402
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


def main() -> int:
    p = argparse.ArgumentParser()
    p.add_argument("labels", help="labels.npy of bench.py --dump-outputs ([B, H, W] uint8)")
    p.add_argument("--camera", default="640x480", help="camera the maps were letterboxed from")
    p.add_argument("--crop", default=None, help="valid region WIDTHxHEIGHT (default: the camera's letterbox)")
    p.add_argument("--cap", type=int, default=0, help="run slots per frame (0: Config default)")
    a = p.parse_args()
    from semantic_segmentation_server_amd.config import Config
    cap = a.cap or Config().mask_max_runs
    lab = np.ascontiguousarray(np.load(a.labels), np.uint8)
    B, H, W = lab.shape
    if a.crop:
        cw, ch = (int(v) for v in a.crop.split("x"))
    else:
        from semantic_segmentation_server_amd.ops import reference_ops as R
        cam_w, cam_h = (int(v) for v in a.camera.split("x"))
        cw, ch = R.letterbox_luts(cam_w, cam_h, W, H)[4:6]
    runs = [int(MR.encode(l, cw, ch, 2)[0]) for l in lab]
    print(f"{B} maps {H} x {W}, crop {cw} x {ch}: runs per frame min {min(runs)} median "
          f"{int(np.median(runs))} max {max(runs)}; distinct labels {np.unique(lab).tolist()}")
    dev = torch.device("cuda")
    out = {"maps": B, "crop": [cw, ch], "runs_min": min(runs), "runs_median": int(np.median(runs)),
           "runs_max": max(runs), "cap": cap}
    post = DevicePostprocess(dev, H, W, colormap_for("pascal"), 64, bins=21)
    for b in (B, 1):
        d = torch.from_numpy(lab[:b]).to(dev)
        words = torch.zeros((b, 4 + cap), dtype=torch.int32, device=dev)
        ws = torch.zeros(max(4, hip_ops.mask_rle_workspace_bytes(b, ch, cw)), dtype=torch.uint8, device=dev)

        def enc():
            hip_ops.mask_rle(d, words, ws, B=b, H=H, W=W, crop_h=ch, crop_w=cw, cap=cap)

        enc()
        torch.cuda.synchronize()
        got = words.cpu().numpy().view(np.uint32)
        for i in range(b):
            want = MR.encode(lab[i], cw, ch, cap)
            u = MR.used_words(want)
            assert np.array_equal(got[i, :u], want[:u]), f"frame {i}: device words differ from the spec"
        lo, med = graph_us(enc)
        plo, pmed = graph_us(lambda: post.run(d, cw, ch, 0.05 * H * W))
        print(f"B = {b:2d}: mask_rle {lo:7.1f} us min {med:7.1f} us median per batch; "
              f"postprocess {plo:7.1f} / {pmed:7.1f} us")
        out[f"mask_rle_us_b{b}"] = round(med, 1)
        out[f"mask_rle_us_min_b{b}"] = round(lo, 1)
        out[f"postprocess_us_b{b}"] = round(pmed, 1)
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
