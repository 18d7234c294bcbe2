"""Single configuration dataclass + CLI.

Reference flags (``sem_seg_server.py:236-260``) are kept with the same names and
defaults: ``--model``, ``--labels``, ``--keep_aspect_ratio`` (default True — made a
real toggle via ``--no_keep_aspect_ratio``; the reference's ``store_true`` plus
``set_defaults(True)`` could never turn it off), ``--camera_idx`` (1),
``--num_detections`` (3), ``--min_area_ratio`` (0.05). The reference's hard-coded
port 50051 (``:281``) and pool size 10 (``:272``) become ``--port`` and
``--max_workers``. Everything else is new.
"""
from __future__ import annotations

import argparse
import dataclasses
import os
from dataclasses import dataclass, field
from typing import List, Optional

from .labels import CITYSCAPES_LABELS, PASCAL_LABELS


PIXEL_FORMATS = ("bgr", "yuyv", "uyvy")


@dataclass
class Config:
    # --- reference flags ---
    model: Optional[str] = None            # optional weights file (.pt state_dict / .safetensors)
    labels: str = PASCAL_LABELS
    keep_aspect_ratio: bool = True
    camera_idx: int = 1
    num_detections: int = 3
    min_area_ratio: float = 0.05
    # --- serving ---
    port: int = 50051
    host: str = "[::]"
    max_workers: int = 10
    buffer_max: Optional[int] = 4096       # None = unbounded (reference semantics)
    # --- sources ---
    source: str = "synthetic"              # synthetic | file | camera
    source_path: Optional[str] = None
    camera_width: int = 640
    camera_height: int = 480
    streams: int = 1                       # camera streams per rank
    fps_limit: Optional[float] = None
    pixel_format: str = "bgr"              # bgr | yuyv | uyvy (raw packed 4:2:2, converted on the device)
    # --- model ---
    arch: str = "mnv2"                     # mnv2 | resnet50
    num_classes: int = 21
    dataset: str = "pascal"                # palette for the mask stage
    width_mult: float = 1.0
    output_stride: int = 16
    aspp: str = "full"                     # full | mobile
    input_size: int = 513
    seed: int = 0
    # --- execution ---
    backend: str = "hip"                   # hip | torch
    dtype: str = "bf16"                    # bf16 | fp32 | int8
    device: str = "auto"                   # auto | cpu | cuda
    batch: int = 1                         # frames per rank per step
    graph: bool = True                     # hipGraph capture of the per-step device work
    contour_mode: str = "fast"             # fast (device CCL stats) | exact (host tracer)
    max_segments: int = 64                 # per-frame record capacity on device
    serve_masks: bool = False              # run-length encode every label map (v2 GetSegmentationMask)
    mask_max_runs: int = 32768             # run slots per frame; more runs truncate the mask
    serve_regions: bool = False            # connected same-class regions of every label map (v2 GetClassRegions)
    max_regions: int = 64                  # region records per frame (1 .. 256), largest first
    region_min_area_ratio: float = 0.002   # smallest region served, as a share of input_size^2
    region_classes: Optional[str] = None   # comma list of class ids / label names; None: all but 0
    serve_confidence: bool = False         # per-pixel confidence on the device, served per class region
    track_regions: bool = False            # match the regions of consecutive frames: track_id, age per region
    track_min_overlap: float = 0.25        # overlap / smaller region that continues a track, in (0, 1]
    serve_zones: bool = False              # class x zone pixel counts of every label map (v2 GetZoneOccupancy)
    zones: Optional[str] = None            # zone file (JSON, postprocess/zones.py); None: the frame zone alone
    serve_presence: bool = False           # region x zone pixel overlap, per-track dwell (v2 GetZonePresence)
    presence_min_share: float = 0.5        # share of a region's pixels inside a zone that puts it inside, in (0, 1]
    serve_events: bool = False             # enter / leave events of the tracks per zone, every frame (v2 GetZoneEvents)
    max_events: int = 64                   # events stored per frame (1 .. 4096); the true count is always reported
    event_log: int = 4096                  # events kept per stream for GetZoneEvents (at least max_events)
    stable_labels: int = 0                 # hold each pixel's label until another is seen N frames in a row (0: off; 2 .. 255)
    stable_min_confidence: float = 0.0     # ignore observations below this confidence, in [0, 1] (0: no gate)
    smooth_labels: int = 0                 # majority label of each pixel's (2R+1)^2 window, ahead of stable_labels (0: off; 1 .. 3)
    # --- distributed ---
    gpus: int = 1
    ingest: str = "local"                  # local (per-rank H2D) | scatter (rank-0 RCCL scatter)
    gather: str = "auto"                   # record gather to rank 0: auto (= host) | host
                                           # (pinned host + gloo) | rccl (RCCL over xGMI)
    # --- observability ---
    profile: bool = False
    metrics_dump: Optional[str] = None
    log_level: str = "INFO"
    inject_fault: Optional[str] = None     # "rank:step" fault injection for tests
    rank_timeout: float = 300.0            # process-group collective timeout (s)
    degrade: bool = True                   # rank 0 keeps serving alone when a peer rank is lost
    debug_dump: Optional[str] = None       # directory for annotated PNG frames (reference :196-205)
    debug_every: int = 0                   # dump every N-th frame (0 = off)
    debug_sync: bool = False               # HIP_LAUNCH_BLOCKING=1, eager launches
    supervise: bool = True                 # CLI: GPU work in supervised worker processes (one per GPU)

    def __post_init__(self):
        if self.pixel_format not in PIXEL_FORMATS:
            raise ValueError(f"--pixel_format must be one of {', '.join(PIXEL_FORMATS)}, "
                             f"got {self.pixel_format!r}")
        if self.serve_confidence and not (self.serve_regions or self.serve_zones):
            raise ValueError("--serve_confidence requires --serve_regions or --serve_zones: the "
                             "confidence is served per class region (v2 GetClassRegions) or per "
                             "class and zone (v2 GetZoneOccupancy)")
        if self.zones and not self.serve_zones:
            raise ValueError(f"--zones {self.zones} requires --serve_zones: the zones are served by "
                             "v2 GetZoneOccupancy")
        if self.track_regions and not self.serve_regions:
            raise ValueError("--track_regions requires --serve_regions: a track is the identity of a "
                             "class region across frames (v2 GetClassRegions)")
        if self.track_regions and not 0.0 < float(self.track_min_overlap) <= 1.0:
            raise ValueError(f"--track_min_overlap {self.track_min_overlap} outside (0, 1]")
        if self.serve_presence and not (self.serve_regions and self.serve_zones):
            raise ValueError("--serve_presence requires --serve_regions and --serve_zones: presence is "
                             "the overlap of the class regions with the zones (v2 GetZonePresence)")
        if self.serve_presence and not 0.0 < float(self.presence_min_share) <= 1.0:
            raise ValueError(f"--presence_min_share {self.presence_min_share} outside (0, 1]")
        if self.serve_events:
            if not (self.serve_presence and self.track_regions):
                raise ValueError("--serve_events requires --serve_presence and --track_regions: an event "
                                 "is an edge of a track's dwell in a zone (v2 GetZoneEvents)")
            from .postprocess import events as EV
            EV.check_geometry(int(self.max_events))
            if int(self.event_log) < int(self.max_events):
                raise ValueError(f"--event_log {self.event_log} is smaller than --max_events "
                                 f"{self.max_events}: the log holds at least one frame's events")
        if int(self.stable_labels) != 0 and not 2 <= int(self.stable_labels) <= 255:
            raise ValueError(f"--stable_labels {self.stable_labels} outside 2 .. 255 (0: off)")
        if not 0.0 <= float(self.stable_min_confidence) <= 1.0:
            raise ValueError(f"--stable_min_confidence {self.stable_min_confidence} outside [0, 1]")
        if float(self.stable_min_confidence) > 0.0 and not int(self.stable_labels):
            raise ValueError(f"--stable_min_confidence {self.stable_min_confidence} requires "
                             "--stable_labels: it gates the observations of the label stabilisation")
        if float(self.stable_min_confidence) > 0.0 and not self.serve_confidence:
            raise ValueError(f"--stable_min_confidence {self.stable_min_confidence} requires "
                             "--serve_confidence: the gate reads the per-pixel confidence plane")
        if not 0 <= int(self.smooth_labels) <= 3:
            raise ValueError(f"--smooth_labels {self.smooth_labels} outside 1 .. 3 (0: off)")
        if self.pixel_format != "bgr":
            if self.camera_width % 2:
                raise ValueError(f"--pixel_format {self.pixel_format} packs pixels in pairs: "
                                 f"--camera_width {self.camera_width} must be even")
            if self.ingest == "scatter":
                raise ValueError(f"--ingest scatter is not supported with --pixel_format "
                                 f"{self.pixel_format}: the scatter path moves BGR frames only; "
                                 "use --ingest local")

    @property
    def frame_channels(self) -> int:
        """Bytes per pixel of an ingested frame: 3 (BGR) or 2 (packed 4:2:2)."""
        return 3 if self.pixel_format == "bgr" else 2

    @property
    def min_area(self) -> float:
        return self.min_area_ratio * self.input_size * self.input_size

    def replace(self, **kw) -> "Config":
        return dataclasses.replace(self, **kw)

    def resolve_dataset_defaults(self) -> "Config":
        if self.dataset == "cityscapes" and self.labels == PASCAL_LABELS:
            self.labels = CITYSCAPES_LABELS
        return self


def add_args(p: argparse.ArgumentParser) -> argparse.ArgumentParser:
    d = Config()
    # reference flags, same names/defaults
    p.add_argument("--model", default=d.model, help="optional weights file (torch state_dict or safetensors); random init if omitted")
    p.add_argument("--labels", default=d.labels, help="label file path")
    p.add_argument("--keep_aspect_ratio", dest="keep_aspect_ratio", action="store_true",
                   help="keep the image aspect ratio when resizing, padding bottom/right with zeros (default)")
    p.add_argument("--no_keep_aspect_ratio", dest="keep_aspect_ratio", action="store_false",
                   help="stretch frames to the model input instead of letterboxing")
    p.set_defaults(keep_aspect_ratio=True)
    p.add_argument("--camera_idx", type=int, default=d.camera_idx, help="index of the video source")
    p.add_argument("--num_detections", type=int, default=d.num_detections, help="number of detections to return")
    p.add_argument("--min_area_ratio", type=float, default=d.min_area_ratio, help="segment centroid min area ratio")
    # new
    p.add_argument("--port", type=int, default=d.port)
    p.add_argument("--host", default=d.host)
    p.add_argument("--max_workers", type=int, default=d.max_workers)
    p.add_argument("--buffer_max", type=int, default=d.buffer_max, help="result buffer bound; 0 = unbounded")
    p.add_argument("--source", choices=["synthetic", "file", "camera"], default=d.source)
    p.add_argument("--source_path", default=d.source_path)
    p.add_argument("--camera_width", type=int, default=d.camera_width)
    p.add_argument("--camera_height", type=int, default=d.camera_height)
    p.add_argument("--streams", type=int, default=d.streams)
    p.add_argument("--fps_limit", type=float, default=d.fps_limit)
    p.add_argument("--pixel_format", choices=list(PIXEL_FORMATS), default=d.pixel_format,
                   help="format of the ingested frames: bgr, or raw packed 4:2:2 (yuyv | uyvy) "
                        "uploaded at 2 bytes per pixel and converted to BGR on the device")
    p.add_argument("--arch", choices=["mnv2", "resnet50"], default=d.arch)
    p.add_argument("--num_classes", type=int, default=d.num_classes)
    p.add_argument("--dataset", choices=["pascal", "cityscapes"], default=d.dataset)
    p.add_argument("--width_mult", type=float, default=d.width_mult)
    p.add_argument("--output_stride", type=int, default=d.output_stride)
    p.add_argument("--aspp", choices=["full", "mobile"], default=d.aspp)
    p.add_argument("--input_size", type=int, default=d.input_size)
    p.add_argument("--seed", type=int, default=d.seed)
    p.add_argument("--backend", choices=["hip", "torch"], default=d.backend)
    p.add_argument("--dtype", choices=["bf16", "fp32", "int8"], default=d.dtype)
    p.add_argument("--device", default=d.device)
    p.add_argument("--batch", type=int, default=d.batch)
    p.add_argument("--graph", dest="graph", action="store_true")
    p.add_argument("--no-graph", "--no_graph", dest="graph", action="store_false")
    p.set_defaults(graph=d.graph)
    p.add_argument("--contour_mode", choices=["fast", "exact"], default=d.contour_mode)
    p.add_argument("--max_segments", type=int, default=d.max_segments)
    p.add_argument("--serve_masks", action="store_true",
                   help="run-length encode every frame's label map on the device and serve the "
                        "latest one per stream (v2 GetSegmentationMask); one GPU per process group")
    p.add_argument("--mask_max_runs", type=int, default=d.mask_max_runs,
                   help="run slots per frame of the mask encoder; a frame with more runs is "
                        "served truncated")
    p.add_argument("--serve_regions", action="store_true",
                   help="find the 8-connected regions of every class in each frame's label map on "
                        "the device and serve the latest ones per stream with box, centroid and "
                        "area (v2 GetClassRegions); one GPU per process group")
    p.add_argument("--max_regions", type=int, default=d.max_regions,
                   help="region records per frame, largest first (1 .. 256)")
    p.add_argument("--region_min_area_ratio", type=float, default=d.region_min_area_ratio,
                   help="smallest region served, as a share of the model input's pixels")
    p.add_argument("--region_classes", default=d.region_classes,
                   help="comma list of class ids or label names whose regions are served "
                        "(default: every class but 0)")
    p.add_argument("--serve_confidence", action="store_true",
                   help="compute the winning class's softmax probability of every pixel on the "
                        "device and serve its mean per class region (v2 GetClassRegions "
                        "confidence) and per class and zone (v2 GetZoneOccupancy); requires "
                        "--serve_regions or --serve_zones")
    p.add_argument("--track_regions", action="store_true",
                   help="match the class regions of each stream's consecutive frames by pixel "
                        "overlap on the device and serve a track id and an age per region (v2 "
                        "GetClassRegions track_id, age); requires --serve_regions")
    p.add_argument("--track_min_overlap", type=float, default=d.track_min_overlap,
                   help="smallest overlap, as a share of the smaller of two regions, that "
                        "continues a track (0 < ratio <= 1)")
    p.add_argument("--serve_zones", action="store_true",
                   help="count the pixels of every class inside every zone of each frame's label "
                        "map on the device and serve the latest counts per stream (v2 "
                        "GetZoneOccupancy); zone 0 is the whole frame; one GPU per process group")
    p.add_argument("--zones", default=d.zones, metavar="FILE.json",
                   help="zone file: up to 32 named polygons or rectangles in normalised camera "
                        "coordinates; requires --serve_zones (without it only the frame zone is served)")
    p.add_argument("--serve_presence", action="store_true",
                   help="count the pixels of every class region inside every zone on the device and "
                        "serve them per stream (v2 GetZonePresence); with --track_regions also how "
                        "many frames each track has been inside each zone; requires --serve_regions "
                        "and --serve_zones")
    p.add_argument("--presence_min_share", type=float, default=d.presence_min_share,
                   help="share of a region's pixels inside a zone from which the region counts as "
                        "inside it (0 < share <= 1)")
    p.add_argument("--serve_events", action="store_true",
                   help="detect on the device, for every processed frame, the tracks that entered or "
                        "left a zone (and were born or ended) and serve them as a log per stream (v2 "
                        "GetZoneEvents); requires --serve_presence and --track_regions")
    p.add_argument("--max_events", type=int, default=d.max_events, metavar="E",
                   help="with --serve_events: events stored per frame (1 .. 4096); a frame with more "
                        "is truncated and the true count reported")
    p.add_argument("--event_log", type=int, default=d.event_log, metavar="N",
                   help="with --serve_events: events kept per stream for GetZoneEvents (at least "
                        "--max_events)")
    p.add_argument("--stable_labels", type=int, default=d.stable_labels, metavar="N",
                   help="hold each pixel's label until a different label has been seen for N "
                        "consecutive frames of its stream (2 .. 255), on the device ahead of all "
                        "post-processing; records, masks, regions, tracks, zones and presence see "
                        "the stabilised maps (0: off)")
    p.add_argument("--stable_min_confidence", type=float, default=d.stable_min_confidence,
                   help="with --stable_labels: ignore an observation whose confidence is below "
                        "this (0 .. 1; 0: no gate); requires --serve_confidence")
    p.add_argument("--smooth_labels", type=int, default=d.smooth_labels, metavar="R",
                   help="replace each pixel's label by the most frequent label of its (2R+1) x (2R+1) "
                        "window (1 .. 3), on the device ahead of --stable_labels and all "
                        "post-processing; records, masks, regions, tracks, zones and presence see "
                        "the smoothed maps (0: off)")
    p.add_argument("--gpus", type=int, default=d.gpus)
    p.add_argument("--ingest", choices=["local", "scatter"], default=d.ingest)
    p.add_argument("--gather", choices=["auto", "rccl", "host"], default=d.gather,
                   help="per-step record gather to rank 0: pinned host memory over gloo "
                        "(auto; no GPU time) or RCCL over xGMI (rccl)")
    p.add_argument("--profile", action="store_true")
    p.add_argument("--metrics_dump", default=d.metrics_dump)
    p.add_argument("--log_level", default=d.log_level)
    p.add_argument("--inject_fault", default=d.inject_fault)
    p.add_argument("--rank_timeout", type=float, default=d.rank_timeout)
    p.add_argument("--no_degrade", dest="degrade", action="store_false",
                   help="exit instead of serving from rank 0 alone when a peer rank is lost")
    p.add_argument("--debug_dump", default=d.debug_dump,
                   help="write annotated PNG frames here (contours, centroids, labels)")
    p.add_argument("--debug_every", type=int, default=d.debug_every)
    p.add_argument("--debug_sync", action="store_true",
                   help="synchronous kernel launches (HIP_LAUNCH_BLOCKING=1, no hipGraph) so a "
                        "faulting kernel is reported at its own launch")
    p.add_argument("--no_supervise", dest="supervise", action="store_false",
                   help="run the GPU pipeline in the serving process itself (no restart of a "
                        "faulted worker)")
    return p


def apply_debug_env(cfg: Config) -> Config:
    """--debug_sync: must run before anything initialises the HIP runtime (the
    variable is read once, at runtime init). hipGraph capture is turned off too:
    a graph replays its kernels as one submission, which would hide the culprit."""
    if cfg.debug_sync:
        os.environ["HIP_LAUNCH_BLOCKING"] = "1"
        cfg = dataclasses.replace(cfg, graph=False)
    return cfg


def from_args(args: argparse.Namespace) -> Config:
    kw = {f.name: getattr(args, f.name) for f in dataclasses.fields(Config) if hasattr(args, f.name)}
    if kw.get("buffer_max") == 0:
        kw["buffer_max"] = None
    return Config(**kw).resolve_dataset_defaults()


def parse(argv: Optional[List[str]] = None) -> Config:
    p = add_args(argparse.ArgumentParser(description="MI355X semantic segmentation server"))
    return from_args(p.parse_args(argv))
