"""Example client and RPC latency benchmark.

``run()`` mirrors the reference client (``sem_seg_client.py:11-40``): an insecure
channel to ``localhost:50051`` and an endless loop alternating
``GetCameraResolution`` and ``GetSegmentedObjects``, printing the responses; on an
``RpcError`` it prints details and code and exits with status 1. ``--count``
bounds the loop (the reference's is infinite with no sleep).

``rpc_latency()`` measures the p50/p99 of ``GetSegmentedObjects`` — the latency
half of the headline metric (BASELINE.json).
"""
from __future__ import annotations

import argparse
import sys
import time
from typing import Dict, List, Optional

import grpc
import numpy as np

from .api import proto as P
from .api.service import SemanticSegmentationStub, SemanticSegmentationV2Stub


def get_camera_resolution(stub):
    try:
        response = stub.GetCameraResolution(P.Empty())
        print("Camera resolution fetched.")
        return response
    except grpc.RpcError as err:
        print(err.details())
        print("{}, {}".format(err.code().name, err.code().value))
        sys.exit(1)


def get_detected_objects(stub):
    try:
        response = stub.GetSegmentedObjects(P.Empty())
        print("Detected object(s) fetched.")
        return response
    except grpc.RpcError as err:
        print(err.details())
        print("{}, {}".format(err.code().name, err.code().value))
        sys.exit(1)


def run(target: str = "localhost:50051", count: Optional[int] = None) -> None:
    with grpc.insecure_channel(target) as channel:
        stub = SemanticSegmentationStub(channel)
        i = 0
        while count is None or i < count:
            print(get_camera_resolution(stub))
            print(get_detected_objects(stub))
            i += 1


def rpc_latency(target: str, n: int = 2000, warmup: int = 200) -> Dict[str, float]:
    """Sequential GetSegmentedObjects round trips over one channel."""
    with grpc.insecure_channel(target) as channel:
        stub = SemanticSegmentationStub(channel)
        grpc.channel_ready_future(channel).result(timeout=30)
        for _ in range(warmup):
            stub.GetSegmentedObjects(P.Empty())
        lat: List[float] = []
        for _ in range(n):
            t0 = time.perf_counter()
            stub.GetSegmentedObjects(P.Empty())
            lat.append((time.perf_counter() - t0) * 1e3)
    a = np.asarray(lat)
    return {"p50_ms": float(np.percentile(a, 50)), "p99_ms": float(np.percentile(a, 99)),
            "mean_ms": float(a.mean()), "n": n}


def fetch_mask(target: str, stream: int = 0):
    """(SegmentationMask message, decoded uint8 [height, width] label map; pixels a truncated
    mask does not cover are 255) of the stream's latest frame (v2 GetSegmentationMask)."""
    from .postprocess import mask_rle
    with grpc.insecure_channel(target) as ch:
        m = SemanticSegmentationV2Stub(ch).GetSegmentationMask(P.MaskRequest(stream_id=stream))
    return m, mask_rle.from_wire(m.run_labels, m.run_lengths, m.width, m.height,
                                 allow_truncated=m.truncated)


def print_mask(m, lab: np.ndarray, labels: Dict[int, str]) -> None:
    from .labels import label_name
    print("stream {} frame {} ts {:.3f}: mask {} x {} (model {} x {}), {} runs{}".format(
        m.stream_id, m.frame_id, m.timestamp, m.width, m.height, m.model_width, m.model_height,
        m.total_runs, " (truncated to {})".format(len(m.run_labels)) if m.truncated else ""))
    ids, counts = np.unique(lab, return_counts=True)
    for i, c in sorted(zip(ids.tolist(), counts.tolist()), key=lambda t: -t[1]):
        name = "(not covered)" if m.truncated and i == 255 else label_name(labels, i)
        print("  {:>3} {:<20} {:>8} px  {:5.1f} %".format(i, name, c, 100.0 * c / lab.size))


def fetch_regions(target: str, stream: int = 0, max_regions: int = 0):
    """The ClassRegions message of the stream's latest frame (v2 GetClassRegions)."""
    with grpc.insecure_channel(target) as ch:
        return SemanticSegmentationV2Stub(ch).GetClassRegions(
            P.RegionRequest(stream_id=stream, max_regions=max_regions))


def print_regions(m) -> None:
    print("stream {} frame {} ts {:.3f}: {} regions in {} x {} (model {} x {}){}".format(
        m.stream_id, m.frame_id, m.timestamp, m.total_regions, m.width, m.height, m.model_width,
        m.model_height, " (truncated to {})".format(len(m.regions)) if m.truncated else ""))
    for r in m.regions:
        print("  {:>3} {:<20} {:>8} px  area {:.4f}  centre ({:.3f}, {:.3f})  box ({:.3f}, {:.3f}) - "
              "({:.3f}, {:.3f})".format(r.class_id, r.label, r.pixels, r.area, r.cx, r.cy, r.x_min,
                                       r.y_min, r.x_max, r.y_max) +
              ("  conf {:.3f}".format(r.confidence) if m.has_confidence else "") +
              ("  track {:>5}  age {:>5}".format(r.track_id, r.age) if m.has_tracks else ""))


def fetch_zones(target: str, stream: int = 0):
    """The ZoneOccupancy message of the stream's latest frame (v2 GetZoneOccupancy)."""
    with grpc.insecure_channel(target) as ch:
        return SemanticSegmentationV2Stub(ch).GetZoneOccupancy(P.ZoneRequest(stream_id=stream))


def print_zones(m) -> None:
    print("stream {} frame {} ts {:.3f}: {} zones in {} x {} (model {} x {})".format(
        m.stream_id, m.frame_id, m.timestamp, len(m.zones), m.width, m.height, m.model_width,
        m.model_height))
    for z in m.zones:
        print("  zone {:>2} {:<16} {:>8} px  area {:.4f}".format(z.index, z.name, z.pixels, z.area))
        for c in z.classes:
            print("    {:<16} {:>3} {:<20} {:>8} px  share {:.4f}".format(
                z.name, c.class_id, c.label, c.pixels, c.share) +
                  ("  conf {:.3f}".format(c.confidence) if m.has_confidence else ""))


def fetch_presence(target: str, stream: int = 0):
    """The ZonePresence message of the stream's latest frame (v2 GetZonePresence)."""
    with grpc.insecure_channel(target) as ch:
        return SemanticSegmentationV2Stub(ch).GetZonePresence(P.PresenceRequest(stream_id=stream))


def print_presence(m) -> None:
    print("stream {} frame {} ts {:.3f}: {} regions in {} x {} (model {} x {}), min share {:.3f}".format(
        m.stream_id, m.frame_id, m.timestamp, len(m.regions), m.width, m.height, m.model_width,
        m.model_height, m.min_share))
    for r in m.regions:
        print("  region {:>3} {:>3} {:<20} {:>8} px  root {:>8}".format(
            r.index, r.class_id, r.label, r.pixels, r.root) +
              ("  track {:>5}  age {:>5}".format(r.track_id, r.age) if m.has_tracks else ""))
        for h in r.zones:
            print("    zone {:>2} {:<16} {:>8} px  share {:.4f}  {}".format(
                h.index, h.name, h.pixels, h.share, "inside " if h.inside else "outside") +
                  ("  dwell {:>5}".format(h.dwell) if m.has_tracks else ""))


def fetch_events(target: str, stream: int = 0, after_seq: int = 0, max_events: int = 0, zones=()):
    """The ZoneEvents message of the stream's log after ``after_seq`` (v2 GetZoneEvents)."""
    with grpc.insecure_channel(target) as ch:
        return SemanticSegmentationV2Stub(ch).GetZoneEvents(
            P.EventRequest(stream_id=stream, after_seq=after_seq, max_events=max_events, zones=list(zones)))


def print_events(m) -> None:
    """One line per event."""
    if m.lost:
        print("stream {}: {} events lost (they fell out of the log before this poll)".format(m.stream_id, m.lost))
    for e in m.events:
        print("stream {} seq {:>8} epoch {:>2} frame {:>8} ts {:.3f}  {} zone {:>2} {:<16} track {:>5}  "
              "{:>3} {:<20} root {:>8}  {}{}".format(
                  m.stream_id, e.seq, e.epoch, e.frame_id, e.timestamp,
                  "ENTER" if e.kind == 1 else "LEAVE", e.zone, e.zone_name, e.track_id, e.class_id,
                  e.label, e.root,
                  "{:>8} px".format(e.pixels) if e.kind == 1 else "after {:>5} frames".format(e.dwell),
                  ("  (track begins)" if e.kind == 1 else "  (track ends)") if e.track_edge else ""))


def follow_events(target: str, stream: int = 0, follow: bool = False, period_s: float = 0.2,
                  polls: int = None) -> int:
    """Print the stream's log from its oldest kept event; with ``follow`` keep polling with the
    cursor (``polls``: stop after that many polls)."""
    seq, n = 0, 0
    while True:
        m = fetch_events(target, stream, seq)
        print_events(m)
        more = m.next_seq != seq
        seq, n = m.next_seq, n + 1
        if (not follow and not more) or (polls is not None and n >= polls):
            return 0
        if not more:
            time.sleep(period_s)


def main(argv=None) -> int:
    p = argparse.ArgumentParser(description="sem_seg_server example client")
    p.add_argument("--target", default="localhost:50051")
    p.add_argument("--count", type=int, default=None)
    p.add_argument("--latency", action="store_true", help="measure GetSegmentedObjects latency")
    p.add_argument("--stats", action="store_true", help="print v2 GetStats")
    p.add_argument("--mask", nargs="?", type=int, const=0, default=None, metavar="STREAM",
                   help="fetch the stream's latest label mask (server run with --serve_masks), "
                        "decode it and print per-class pixel counts")
    p.add_argument("--mask_out", default=None, metavar="PATH.npy",
                   help="with --mask: save the decoded uint8 label map")
    p.add_argument("--labels", default=None, help="label file for --mask (default: Pascal VOC)")
    p.add_argument("--regions", nargs="?", type=int, const=0, default=None, metavar="STREAM",
                   help="fetch the class regions of the stream's latest frame (server run with "
                        "--serve_regions) and print one line per region")
    p.add_argument("--zones_of", nargs="?", type=int, const=0, default=None, metavar="STREAM",
                   help="fetch the zone occupancy of the stream's latest frame (server run with "
                        "--serve_zones) and print, per zone, one line per class present")
    p.add_argument("--presence", nargs="?", type=int, const=0, default=None, metavar="STREAM",
                   help="fetch the zone presence of the stream's latest frame (server run with "
                        "--serve_presence) and print one line per region and zone hit")
    p.add_argument("--events", nargs="?", type=int, const=0, default=None, metavar="STREAM",
                   help="print the stream's zone events, one line each (server run with --serve_events)")
    p.add_argument("--follow", action="store_true",
                   help="with --events: keep polling with the cursor and print events as they come")
    a = p.parse_args(argv)
    if a.events is not None:
        try:
            return follow_events(a.target, a.events, a.follow)
        except grpc.RpcError as err:
            print(err.details())
            print("{}, {}".format(err.code().name, err.code().value))
            return 1
    if a.presence is not None:
        try:
            m = fetch_presence(a.target, a.presence)
        except grpc.RpcError as err:
            print(err.details())
            print("{}, {}".format(err.code().name, err.code().value))
            return 1
        print_presence(m)
        return 0
    if a.zones_of is not None:
        try:
            m = fetch_zones(a.target, a.zones_of)
        except grpc.RpcError as err:
            print(err.details())
            print("{}, {}".format(err.code().name, err.code().value))
            return 1
        print_zones(m)
        return 0
    if a.regions is not None:
        try:
            m = fetch_regions(a.target, a.regions)
        except grpc.RpcError as err:
            print(err.details())
            print("{}, {}".format(err.code().name, err.code().value))
            return 1
        print_regions(m)
        return 0
    if a.mask is not None:
        from .labels import PASCAL_LABELS, load_labels
        try:
            m, lab = fetch_mask(a.target, a.mask)
        except grpc.RpcError as err:
            print(err.details())
            print("{}, {}".format(err.code().name, err.code().value))
            return 1
        print_mask(m, lab, load_labels(a.labels or PASCAL_LABELS))
        if a.mask_out:
            np.save(a.mask_out, lab)
        return 0
    if a.latency:
        print(rpc_latency(a.target))
        return 0
    if a.stats:
        with grpc.insecure_channel(a.target) as ch:
            print(SemanticSegmentationV2Stub(ch).GetStats(P.Empty()))
        return 0
    run(a.target, a.count)
    return 0


if __name__ == "__main__":
    sys.exit(main())
