"""Cost of the zone-event launches (csrc/hip/zone_events.hip): alone on built presence rows, and
at the end of the region / track / zone / presence chain on planted label maps.

    python scripts/events_bench.py [--size 513] [--camera 640x480] [--batch 32]

Alone, at B = 32 as 16 streams of two rows (so every replay of the graph meets the state the
replay before it saved), K = --max_regions and E = --max_events of the default config, for Z = 4
and Z = 32 zones, three cases of rows built by hand (the kernels read nothing else):
  quiet     no event in any frame (every dwell goes on)
  few       two events a frame (two tracks toggle one zone)
  allflip   every entry of every frame leaves every row and every entry enters it
and the all-flip case again at the limits K = 256, R = 33, E = 4096. Each case is checked against
the numpy definition (postprocess/events.py) before it is timed from hipGraph replays
(scripts/zones_bench.py ``graph_us``). The copy kernel to pinned memory is timed with them.

At the end of the chain: class_regions, region_tracks, zone_stats and zone_presence on planted
maps at the headline crop, timed as one graph without and with zone_events as their last launches
(replays of one batch of maps: after the first replay every track goes on, the quiet case).
One JSON line at the end.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from semantic_segmentation_server_amd.ops import hip_ops  # noqa: E402
from semantic_segmentation_server_amd.postprocess import events as EV  # noqa: E402
from semantic_segmentation_server_amd.postprocess import presence as PR  # noqa: E402
from semantic_segmentation_server_amd.postprocess import regions as RG  # noqa: E402
from semantic_segmentation_server_amd.postprocess import synthetic  # noqa: E402
from semantic_segmentation_server_amd.postprocess import zones as ZN  # noqa: E402
from scripts.zones_bench import graph_us, zone_sets  # noqa: E402


def _row(K, R, ids, D, N, cw, ch):
    n = len(ids)
    U = PR.unit(R, True)
    w = np.zeros(PR.frame_words(K, R, True), np.uint32)
    w[:4] = (n, N, cw, ch)
    e = w[4:4 + U * n].reshape(n, U)
    e[:, 0] = (np.uint32(1) << 24) | np.asarray(ids, np.uint32)
    e[:, 1] = ids
    e[:, 2:2 + R] = 100
    e[:, 2 + R:] = D
    return w


def cases(K, R, cw, ch):
    """name -> (row A, row B): the two rows of every stream; a replay meets B as the state."""
    N = cw * ch
    ids = np.arange(1, K + 1, dtype=np.uint32)
    steady = _row(K, R, ids, np.full((K, R), 5, np.uint32), N, cw, ch)
    out = {"quiet": (steady, steady)}
    if R > 1:
        a = np.full((K, R), 5, np.uint32)
        b = a.copy()
        a[:2, 1], b[:2, 1] = 1, 0   # B -> A: two ENTERs; A -> B: two LEAVEs
        out["few"] = (_row(K, R, ids, a, N, cw, ch), _row(K, R, ids, b, N, cw, ch))
    out["allflip"] = (_row(K, R, ids, np.full((K, R), 7, np.uint32), N, cw, ch),
                      _row(K, R, ids + K, np.ones((K, R), np.uint32), N, cw, ch))
    return out


def alone(K, R, E, B, cw, ch):
    dev = torch.device("cuda")
    counts = [2] * (B // 2)
    tables = hip_ops.region_track_tables(counts, dev)
    out = {}
    for name, (ra, rb) in cases(K, R, cw, ch).items():
        rows = torch.from_numpy(np.stack([ra, rb] * (B // 2)).view(np.int32)).to(dev)
        words = torch.zeros((B, EV.frame_words(E)), dtype=torch.int32, device=dev)
        state = torch.zeros(hip_ops.zone_events_state_bytes(len(counts), K, R), dtype=torch.uint8, device=dev)
        host = torch.zeros(words.shape, dtype=torch.int32).pin_memory()

        def run():
            hip_ops.zone_events(rows, words, state, tables, counts=counts, K=K, R=R, E=E)

        run()
        run()   # the second run starts from the state the first one saved: row B
        torch.cuda.synchronize()
        got = words.cpu().numpy().view(np.uint32)
        for i, (prev, cur) in enumerate(((rb, ra), (ra, rb))):
            assert np.array_equal(got[i], EV.events_between(prev, cur, R, E)), f"{name}: device words differ"
        per_frame = got[:, 0].astype(np.int64).mean()
        lo, med = graph_us(run)
        clo, cmed = graph_us(lambda: hip_ops.zone_events_copy_to_host(words, host, E))
        key = f"K{K}_R{R}_E{E}_{name}"
        out[key] = {"events_per_frame": round(float(per_frame), 1), "zone_events_us": round(med, 1),
                    "zone_events_us_min": round(lo, 1), "copy_us": round(cmed, 1)}
        print(f"  K = {K:3d} R = {R:2d} E = {E:4d} {name:>8}: {per_frame:8.1f} events a frame  zone_events {lo:7.1f} us min "
              f"{med:7.1f} us median  copy {clo:6.1f} us min {cmed:6.1f} us median  per {B} frames")
    return out


def chain(lab, cw, ch, C, classes, min_pixels, K, E, q):
    B, H, W = lab.shape
    dev = torch.device("cuda")
    out = {}
    d = torch.from_numpy(lab).to(dev)
    rows = torch.zeros((B, 4 + 6 * K), dtype=torch.int32, device=dev)
    wide = torch.zeros((B, 4 + 8 * K), dtype=torch.int32, device=dev)
    ws = torch.zeros(hip_ops.class_regions_workspace_bytes(B, ch, cw), dtype=torch.uint8, device=dev)
    tws = torch.zeros(hip_ops.region_tracks_workspace_bytes(B, ch, cw, K), dtype=torch.uint8, device=dev)
    counts = [1] * B
    tstate = torch.zeros(hip_ops.region_tracks_state_bytes(B, ch, cw), dtype=torch.uint8, device=dev)
    tables = hip_ops.region_track_tables(counts, dev)
    for zname, zl in zone_sets().items():
        if not zl:
            continue
        R = 1 + len(zl)
        plane = ZN.rasterize(zl, cw, ch, warn=False)
        pl = torch.from_numpy(plane.view(np.int32)).to(dev)
        zwords = torch.zeros((B, ZN.frame_words(R, C)), dtype=torch.int32, device=dev)
        zws = torch.zeros(hip_ops.zone_stats_workspace_bytes(B, R, C), dtype=torch.uint8, device=dev)
        pwords = torch.zeros((B, PR.frame_words(K, R, True)), dtype=torch.int32, device=dev)
        pws = torch.zeros(hip_ops.zone_presence_workspace_bytes(B, ch, cw, True), dtype=torch.uint8, device=dev)
        pstate = torch.zeros(hip_ops.zone_presence_state_bytes(B, K, R), dtype=torch.uint8, device=dev)
        ewords = torch.zeros((B, EV.frame_words(E)), dtype=torch.int32, device=dev)
        estate = torch.zeros(hip_ops.zone_events_state_bytes(B, K, R), dtype=torch.uint8, device=dev)

        def run(events):
            hip_ops.class_regions(d, rows, ws, B=B, H=H, W=W, crop_h=ch, crop_w=cw, classes=classes,
                                  min_pixels=min_pixels, K=K)
            hip_ops.region_tracks(rows, wide, ws, tws, tstate, tables, counts=counts, crop_h=ch, crop_w=cw,
                                  K=K, q=256)
            hip_ops.zone_stats(d, zwords, zws, B=B, H=H, W=W, crop_h=ch, crop_w=cw, R=R, C=C, plane=pl)
            hip_ops.zone_presence(wide, pwords, pws, ws, B=B, crop_h=ch, crop_w=cw, K=K, R=R, plane=pl,
                                  tws=tws, state=pstate, tables=tables, counts=counts, q=q)
            if events:
                hip_ops.zone_events(pwords, ewords, estate, tables, counts=counts, K=K, R=R, E=E)

        # the words of two consecutive runs against the definition
        prev = None
        for _ in range(2):
            run(True)
            torch.cuda.synchronize()
            pw, ew = pwords.cpu().numpy().view(np.uint32), ewords.cpu().numpy().view(np.uint32)
            for i in range(2):
                want = EV.events_between(None if prev is None else prev[i], pw[i], R, E)
                assert np.array_equal(ew[i], want), f"chain {zname} frame {i}: device words differ"
            prev = pw.copy()
        off_lo, off = graph_us(lambda: run(False), reps=10)
        on_lo, on = graph_us(lambda: run(True), reps=10)
        out[zname] = {"chain_us": round(off, 1), "chain_events_us": round(on, 1),
                      "chain_us_min": round(off_lo, 1), "chain_events_us_min": round(on_lo, 1)}
        print(f"  chain {zname:>3} B = {B}: without events {off_lo:7.1f} us min {off:7.1f} us median, with "
              f"{on_lo:7.1f} us min {on:7.1f} us median  (+{on - off:5.1f} us, {on / off:5.3f} x)")
    return out


def main() -> int:
    p = argparse.ArgumentParser()
    p.add_argument("--camera", default="640x480", help="camera the maps were letterboxed from")
    p.add_argument("--size", type=int, default=513, help="map size of the planted maps")
    p.add_argument("--batch", type=int, default=32, help="frames a batch (even)")
    a = p.parse_args()
    from semantic_segmentation_server_amd.config import Config
    from semantic_segmentation_server_amd.ops import reference_ops as R
    cfg = Config()
    H = W = a.size
    cam_w, cam_h = (int(v) for v in a.camera.split("x"))
    cw, ch = R.letterbox_luts(cam_w, cam_h, W, H)[4:6]
    B, K, E = a.batch, cfg.max_regions, cfg.max_events
    out = {"crop": [cw, ch], "B": B, "alone": {}, "chain": {}}
    print(f"zone_events alone, {B} frames as {B // 2} streams of two, crop {cw} x {ch}")
    for Rr in (5, 33):
        out["alone"].update(alone(K, Rr, E, B, cw, ch))
    out["alone"].update({k: v for k, v in alone(256, 33, 4096, B, cw, ch).items() if k.endswith("allflip")})
    rng = np.random.default_rng(0)
    lab = np.stack([synthetic.random_label_map(rng, H, W) for _ in range(B)]).astype(np.uint8)
    print(f"end of the chain, planted maps {H} x {W}, K = {K}, E = {E}")
    out["chain"] = chain(lab, cw, ch, cfg.num_classes, RG.default_classes(cfg.num_classes),
                         RG.min_pixels_for(cfg.region_min_area_ratio, H, W), K, E,
                         PR.quantize(cfg.presence_min_share))
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
