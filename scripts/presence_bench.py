"""Cost of the zone-presence launches (csrc/hip/zone_presence.hip) on real and planted label maps.

    python bench.py --gpus 1 --steps 20 --warmup 5 --dump-outputs DIR
    python scripts/presence_bench.py [DIR/labels.npy] [--camera 640x480] [--crop WxH]

Sets of maps: the dumped ones of the bench model (random-init weights: speckled), if given;
planted piecewise-constant ones (postprocess/synthetic.py); a checkerboard of two classes (two
regions, and no two neighbours share a key: the worst case of the run aggregation). Per set, at
B = 32 and B = 1, for Z = 4 rectangles and Z = 32 overlapping zones, without and with tracking,
the class-region (and tracking) kernels run once, the device words are checked against the numpy
definition (postprocess/presence.py), and the presence launches alone -- with tracking: init,
count and the dwell chain; without: the slot planes, init and count -- are timed from hipGraph
replays (``reps`` launches per graph). ``zone_stats``, the sibling single-pass kernel, is timed at
the same Z in the same call: it is the yardstick. One JSON line at the end.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from semantic_segmentation_server_amd.ops import hip_ops  # noqa: E402
from semantic_segmentation_server_amd.postprocess import presence as PR  # noqa: E402
from semantic_segmentation_server_amd.postprocess import regions as RG  # noqa: E402
from semantic_segmentation_server_amd.postprocess import synthetic  # noqa: E402
from semantic_segmentation_server_amd.postprocess import zones as ZN  # noqa: E402
from scripts.zones_bench import graph_us, zone_sets  # noqa: E402


def measure(name, lab, cw, ch, C, classes, min_pixels, K, q):
    B, H, W = lab.shape
    dev = torch.device("cuda")
    out = {"maps": B, "crop": [cw, ch], "K": K, "min_pixels": min_pixels}
    print(f"{name}: {B} maps {H} x {W}, crop {cw} x {ch}, K = {K}, min_pixels = {min_pixels}")
    sets = {k: v for k, v in zone_sets().items() if v}
    for b in (B, 1):
        d = torch.from_numpy(lab[:b]).to(dev)
        rows = torch.zeros((b, 4 + 6 * K), dtype=torch.int32, device=dev)
        wide = torch.zeros((b, 4 + 8 * K), dtype=torch.int32, device=dev)
        ws = torch.zeros(hip_ops.class_regions_workspace_bytes(b, ch, cw), dtype=torch.uint8, device=dev)
        tws = torch.zeros(hip_ops.region_tracks_workspace_bytes(b, ch, cw, K), dtype=torch.uint8, device=dev)
        counts = [1] * b  # every frame the next one of a stream of its own
        tstate = torch.zeros(hip_ops.region_tracks_state_bytes(b, ch, cw), dtype=torch.uint8, device=dev)
        tables = hip_ops.region_track_tables(counts, dev)
        hip_ops.class_regions(d, rows, ws, B=b, H=H, W=W, crop_h=ch, crop_w=cw, classes=classes,
                              min_pixels=min_pixels, K=K)
        for _ in range(2):  # the second run matches every region to itself: every link is set
            hip_ops.region_tracks(rows, wide, ws, tws, tstate, tables, counts=counts, crop_h=ch, crop_w=cw,
                                  K=K, q=256)
        torch.cuda.synchronize()
        stored = np.minimum(rows.cpu().numpy().view(np.uint32)[:, 0], K)
        print(f"  B = {b:2d}: {stored.mean():.1f} stored regions a frame")
        out[f"stored_b{b}"] = round(float(stored.mean()), 1)
        for zname, zl in sets.items():
            R = 1 + len(zl)
            plane = ZN.rasterize(zl, cw, ch, warn=False)
            pl = torch.from_numpy(plane.view(np.int32)).to(dev)
            zwords = torch.zeros((b, ZN.frame_words(R, C)), dtype=torch.int32, device=dev)
            zws = torch.zeros(hip_ops.zone_stats_workspace_bytes(b, R, C), dtype=torch.uint8, device=dev)
            ylo, ymed = graph_us(lambda: hip_ops.zone_stats(d, zwords, zws, B=b, H=H, W=W, crop_h=ch, crop_w=cw,
                                                            R=R, C=C, plane=pl))
            out[f"zone_stats_us_{zname}_b{b}"] = round(ymed, 1)
            print(f"           zone_stats {zname:>3}         {ylo:7.1f} us min {ymed:7.1f} us median")
            for tracks in (False, True):
                words = torch.zeros((b, PR.frame_words(K, R, tracks)), dtype=torch.int32, device=dev)
                pws = torch.zeros(hip_ops.zone_presence_workspace_bytes(b, ch, cw, tracks), dtype=torch.uint8,
                                  device=dev)
                pstate = torch.zeros(hip_ops.zone_presence_state_bytes(b, K, R), dtype=torch.uint8, device=dev)
                kw = dict(tws=tws, state=pstate, tables=tables, counts=counts, q=q) if tracks else {}

                def run():
                    hip_ops.zone_presence(wide if tracks else rows, words, pws, ws, B=b, crop_h=ch, crop_w=cw,
                                          K=K, R=R, plane=pl, **kw)

                run()
                torch.cuda.synchronize()
                got = words.cpu().numpy().view(np.uint32)
                wrows = wide.cpu().numpy().view(np.uint32)
                for i in range(min(b, 2)):  # the oracle on the first frames (it is the slow part)
                    dw = tab = None
                    if tracks:  # ids from the rows; the dwell state was zero: 1 wherever inside
                        dw, tab = PR.StreamDwell(), RG.decode(wrows[i], tracks=True)
                    want = PR.encode(lab[i], plane, cw, ch, classes, min_pixels, K, R, q, tab=tab, dwell=dw)
                    assert np.array_equal(got[i], want), f"{name} {zname} frame {i}: device words differ"
                lo, med = graph_us(run)
                key = f"zone_presence_us_{zname}{'_tracks' if tracks else ''}_b{b}"
                out[key] = round(med, 1)
                print(f"           zone_presence {zname:>3}{' +tracks' if tracks else '        '} {lo:7.1f} us min "
                      f"{med:7.1f} us median  ({med / ymed:4.2f} x zone_stats)")
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
    if a.crop:
        cw, ch = (int(v) for v in a.crop.split("x"))
    else:
        from semantic_segmentation_server_amd.ops import reference_ops as R
        cam_w, cam_h = (int(v) for v in a.camera.split("x"))
        cw, ch = R.letterbox_luts(cam_w, cam_h, W, H)[4:6]
    classes = RG.default_classes(cfg.num_classes)
    mp = RG.min_pixels_for(cfg.region_min_area_ratio, H, W)
    q = PR.quantize(cfg.presence_min_share)
    out = {name: measure(name, lab, cw, ch, cfg.num_classes, classes, mp, cfg.max_regions, q)
           for name, lab in sets.items()}
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
