"""Per-device inference engine.

Replaces the reference's ``BasicEngine`` (``sem_seg_server.py:18,139,162,264``) plus
the per-frame host post-processing (``:164-192``). One ``Engine`` owns one device:

    uint8 BGR camera frames (B, Hc, Wc, 3)
      [--pixel_format yuyv | uyvy: packed 4:2:2 frames (B, Hc, Wc, 2) -> BGR first]
      -> letterbox/normalise (+ stem conv, fused on the HIP path)
      -> DeepLabv3 backbone + ASPP + logits
      -> bilinear upsample + argmax -> (B, H, W) uint8 labels
      -> contour statistics -> compact per-frame records

Backends:
  * ``hip``   — hand-written gfx950 kernels (``models/hip_model.py``,
                ``postprocess/device.py``); the whole step is captured once into a
                hipGraph (``torch.cuda.CUDAGraph``) with static buffers and replayed.
  * ``torch`` — stock PyTorch-ROCm ops (the "framework floor" baseline and the
                CPU path of config 1); also graph-capturable on GPU.

Post-processing (``contour_mode``):
  * ``fast``  — device CCL + quad-decomposition statistics on the HIP backend,
                numpy/scipy component statistics on CPU (same math);
  * ``exact`` — host C++ Suzuki-Abe tracer on the label maps (oracle).
"""
from __future__ import annotations

import logging
import os
import time
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from ..config import Config
from ..labels import colormap_for, load_labels
from ..models.deeplab import build_model
from ..ops import reference_ops as R
from ..postprocess import reference as PR
from .capture import capture
from .results import RECORD_DTYPE

log = logging.getLogger(__name__)

DTYPES = {"bf16": torch.bfloat16, "fp32": torch.float32, "int8": torch.bfloat16}


def calibration_frames(H: int, W: int, n: int = 8, seed: int = 0) -> torch.Tensor:
    """Letterboxed synthetic camera frames at the model resolution, normalised:
    the calibration batch for random-init weights (BN statistics + class prior),
    drawn from the same distribution the synthetic source serves."""
    from .sources import SyntheticSource
    src = SyntheticSource(640, 480, seed=seed + 101, pool=n)
    frames = torch.from_numpy(np.stack([next(src).image for _ in range(n)]).copy())
    lx, ly, *_ = R.letterbox_luts(640, 480, W, H)
    return R.preprocess(frames, torch.from_numpy(np.array(lx)), torch.from_numpy(np.array(ly)))


def _per_frame(streams, n: int) -> List[int]:
    if isinstance(streams, (int, np.integer)):
        return [int(streams)] * n
    return [int(s) for s in streams]


def resolve_device(spec: str = "auto") -> torch.device:
    if spec == "auto":
        return torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() \
            else torch.device("cpu")
    return torch.device(spec)


class Engine:
    def __init__(self, cfg: Config, device: Optional[torch.device] = None,
                 model: Optional[torch.nn.Module] = None):
        self.cfg = cfg
        from ..utils.tracing import NULL_TRACER
        self.tracer = NULL_TRACER  # Server / bench install a live one with --profile
        self.debug = None
        if cfg.debug_dump and cfg.debug_every > 0:
            from ..utils.debug_dump import DebugDumper
            self.debug = DebugDumper(cfg.debug_dump, cfg.debug_every, colormap_for(cfg.dataset),
                                     load_labels(cfg.labels),
                                     cfg.min_area_ratio * cfg.input_size * cfg.input_size)
        self.device = device or resolve_device(cfg.device)
        self.is_cuda = self.device.type == "cuda"
        self.H = self.W = int(cfg.input_size)
        self.min_area = cfg.min_area
        self.palette = np.ascontiguousarray(colormap_for(cfg.dataset), np.int32)
        if model is None:
            calib = None if cfg.model else calibration_frames(self.H, self.W, seed=cfg.seed)
            model = build_model(cfg.arch, cfg.num_classes, cfg.width_mult, cfg.output_stride,
                                cfg.aspp, cfg.seed, calib_input=calib,
                                calib_device=self.device if self.is_cuda else None)
        self.model = model
        if cfg.model:
            self._load_weights(cfg.model)
        self.model.eval()
        self.backend = cfg.backend if self.is_cuda else "torch"
        if self.backend == "hip" and not self.is_cuda:
            raise RuntimeError("hip backend requires a GPU device")
        self.dtype = DTYPES[cfg.dtype] if self.is_cuda else torch.float32
        self.cam: Optional[Tuple[int, int]] = None
        # captured steps (runtime/capture.py): the static input's, and one per buffer declared
        # with bind_inputs, which also decides everything below (defaults: nothing bound)
        self._static_step = None
        self._bound, self._slot_of, self._bound_graphs = {}, {}, {}  # keyed by data_ptr()
        self._split = self.slot_parallel = self.h2d_on_slot = False
        self.result_stream = self.last_consumed = None
        self.slot_streams: List[torch.cuda.Stream] = []
        self.model_streams: List[torch.cuda.Stream] = []
        self.model_parts = 1
        self.device_index = (self.device.index if self.device.index is not None
                             else torch.cuda.current_device() if self.is_cuda else -1)
        self._hip_model = None
        self._hip_post = None
        # --serve_masks: run slots per frame of the label-mask encoder (0 = off: no kernel,
        # no buffer). mask_packed: the [B, 4 + cap] int32 run words of the last run_device
        # (device post-processing: a static device buffer ordered like the records; CPU: a
        # host tensor); masks: the same of the last step(), uint32 on the host
        self.mask_cap = int(cfg.mask_max_runs) if cfg.serve_masks else 0
        if cfg.serve_masks:
            from ..postprocess import mask_rle as MR
            MR.check_geometry(self.W, self.H, self.mask_cap)  # every crop is within H x W
        self.mask_packed: Optional[torch.Tensor] = None
        self.masks: Optional[np.ndarray] = None
        # --serve_regions: records per frame of the class-region kernels (0 = off: no kernel,
        # no buffer); region_packed / regions: as mask_packed / masks, [B, 4 + 6 cap] words
        # (postprocess/regions.py)
        self.region_cap = int(cfg.max_regions) if cfg.serve_regions else 0
        self.region_mask, self.region_min_pixels = 0, 1
        if cfg.serve_regions:
            from ..labels import parse_class_list
            from ..postprocess import regions as RG
            self.region_mask = (RG.class_mask(parse_class_list(cfg.region_classes, load_labels(cfg.labels)))
                                if cfg.region_classes else RG.default_classes(cfg.num_classes))
            self.region_min_pixels = RG.min_pixels_for(cfg.region_min_area_ratio, self.H, self.W)
            # every crop is within H x W, and holds no more candidates than the whole map
            RG.check_geometry(self.W, self.H, self.region_min_pixels, self.region_cap)
        self.region_packed: Optional[torch.Tensor] = None
        self.regions: Optional[np.ndarray] = None
        # --serve_confidence: the model also writes a (B, H, W) uint8 confidence plane
        # (reference_ops.upsample_confidence) and a region has a 7th word, sum_conf.
        # conf_plane: the plane of the last run_device / step (a static buffer, like labels)
        self.serve_confidence = bool(getattr(cfg, "serve_confidence", False))
        serve_zones = bool(getattr(cfg, "serve_zones", False))
        if self.serve_confidence and not (cfg.serve_regions or serve_zones):
            raise ValueError("--serve_confidence requires --serve_regions or --serve_zones")
        self.region_words = 7 if self.serve_confidence else 6
        self.conf_plane: Optional[torch.Tensor] = None
        # --serve_zones: class x zone pixel counts of every label map (postprocess/zones.py).
        # zone_rows: R = 1 + the zones of --zones (0 = off: no kernel, no buffer); the zones are
        # loaded and checked here, rasterised per camera geometry in set_camera. zone_packed /
        # zones: as mask_packed / masks, [B, 4 + R C] words ([B, 4 + 2 R C] with confidence)
        self.zone_rows, self.zone_classes, self.zone_list, self.zone_plane = 0, 0, [], None
        if getattr(cfg, "zones", None) and not serve_zones:
            raise ValueError(f"--zones {cfg.zones} requires --serve_zones")
        if serve_zones:
            from ..postprocess import zones as ZN
            self.zone_list = ZN.load(cfg.zones) if cfg.zones else []
            self.zone_rows, self.zone_classes = 1 + len(self.zone_list), int(cfg.num_classes)
            ZN.check_geometry(self.W, self.H, len(self.zone_list), self.zone_classes)  # every crop is within
        self.zone_conf = bool(self.zone_rows) and self.serve_confidence
        self.zone_packed: Optional[torch.Tensor] = None
        self.zones: Optional[np.ndarray] = None
        self._step_zones = None  # the zone words of the step _step_all issued last
        # --track_regions: every stored region record ends in track_id and age
        # (postprocess/tracks.py), so region_words is two more. On the device the state of the
        # track_streams streams lives in the one DevicePostprocess, and a batch of B frames is
        # laid out by feeder.split_batch(B, track_streams); the host paths keep a StreamTracker
        # per stream id
        self.track_regions = bool(getattr(cfg, "track_regions", False))
        self.track_streams = max(1, int(cfg.streams)) if self.track_regions else 0
        self.track_q = 0
        self._trackers = None
        self._track_ids: Dict[int, int] = {}  # layout position of a stream -> its id
        if self.track_regions:
            if not cfg.serve_regions:
                raise ValueError("--track_regions requires --serve_regions")
            from ..postprocess import tracks as TK
            self.track_q = TK.quantize(cfg.track_min_overlap)
            self._trackers = TK.Trackers(self.track_q)
            self.region_words += 2
        # --serve_presence: pixel overlap of every stored region with every zone row and, with
        # tracks, the dwell of its track in each (postprocess/presence.py). presence_rows: R (0 =
        # off: no kernel, no buffer); presence_packed / presence: as zone_packed / zones,
        # [B, 4 + U region_cap] words. The device dwell state lives in the one DevicePostprocess
        # beside the track state; the host paths keep a StreamDwell per stream id
        self.presence_rows, self.presence_q, self.presence_unit = 0, 0, 0
        self.presence_tracks = False
        self._dwells = None
        if getattr(cfg, "serve_presence", False):
            if not (cfg.serve_regions and serve_zones):
                raise ValueError("--serve_presence requires --serve_regions and --serve_zones")
            from ..postprocess import presence as PR
            self.presence_rows, self.presence_tracks = self.zone_rows, self.track_regions
            self.presence_q = PR.quantize(cfg.presence_min_share)
            self.presence_unit = PR.unit(self.presence_rows, self.presence_tracks)
            PR.check_geometry(self.W, self.H, self.presence_rows - 1, self.region_cap)  # every crop is within
            self._dwells = PR.Dwells()
        self.presence_packed: Optional[torch.Tensor] = None
        self.presence: Optional[np.ndarray] = None
        self._step_presence = None  # the presence words of the step _step_all issued last
        # --serve_events: the enter / leave edges of the presence state between consecutive frames
        # of a stream (postprocess/events.py). event_cap: E, the events stored per frame (0 = off:
        # no kernel, no buffer); events_packed / events: as presence_packed / presence, [B, 4 +
        # 4 E] words. The device state (each stream's last presence row) lives in the one
        # DevicePostprocess; the host paths keep a StreamEvents per stream id
        self.event_cap = 0
        self._events = None
        if getattr(cfg, "serve_events", False):
            if not (getattr(cfg, "serve_presence", False) and self.track_regions):
                raise ValueError("--serve_events requires --serve_presence and --track_regions")
            from ..postprocess import events as EV
            self.event_cap = int(getattr(cfg, "max_events", EV.DEFAULT_MAX_EVENTS))
            EV.check_geometry(self.event_cap)
            self._events = EV.Events(self.event_cap)
        self.events_packed: Optional[torch.Tensor] = None
        self.events: Optional[np.ndarray] = None
        self._step_events = None  # the event words of the step _step_all issued last
        # --stable_labels N: every pixel keeps its label until another has been seen for N
        # consecutive frames of its stream (postprocess/stable.py), ahead of all post-processing:
        # the label maps (and the confidence plane) of a step ARE the stabilised ones. On the
        # device the state of the stable_streams streams lives in the one DevicePostprocess
        # beside the track state, with the same batch layout; the host paths keep a
        # StreamStabilizer per stream id. 0: off -- no kernel, no buffer, nothing changes
        self.stable_frames = int(getattr(cfg, "stable_labels", 0) or 0)
        self.stable_gate, self.stable_streams, self._stabilizers = 0, 0, None
        if float(getattr(cfg, "stable_min_confidence", 0.0) or 0.0) > 0.0 and not self.stable_frames:
            raise ValueError("--stable_min_confidence requires --stable_labels")
        if self.stable_frames:
            from ..postprocess import stable as SB
            self.stable_gate = SB.gate_code(cfg.stable_min_confidence)
            SB.check_params(self.stable_frames, self.stable_gate, self.serve_confidence)
            self.stable_streams = max(1, int(cfg.streams))
            self._stabilizers = SB.Stabilizers(self.stable_frames, self.stable_gate)
        # --smooth_labels R: every pixel takes the most frequent label of its (2R+1)^2 window
        # (postprocess/smooth.py), ahead of the stabilisation and all post-processing: the label
        # maps (and the confidence plane) of a step ARE the smoothed ones. Stateless per frame,
        # so every capture form and every stream layout runs it. 0: off -- no kernel, no buffer
        self.smooth_radius = int(getattr(cfg, "smooth_labels", 0) or 0)
        if self.smooth_radius:
            from ..postprocess import smooth as SM
            SM.check_params(self.smooth_radius)
        # --pixel_format yuyv | uyvy: frames arrive as packed 4:2:2 bytes, (B, Hc, Wc, 2), and
        # are converted to BGR ahead of the model (to_bgr). bgr: no kernel, no buffer
        self.pixel_format = cfg.pixel_format
        self.frame_channels = cfg.frame_channels
        if self.backend == "torch":
            self.model = self.model.to(self.device, self.dtype)
            if self.is_cuda:
                self.model = self.model.to(memory_format=torch.channels_last)
        elif cfg.dtype == "fp32":
            # the HIP kernels compute in bf16/fp16 with fp32 accumulation; an fp32 request
            # must not silently run at lower precision (VERDICT r2 Weak #8)
            raise ValueError("--dtype fp32 is served by --backend torch; the hip backend "
                             "runs bf16 (default) or int8 (--arch resnet50)")
        elif cfg.dtype == "int8":
            if cfg.arch != "resnet50":
                raise ValueError("--dtype int8 is implemented for --arch resnet50 (config 4)")
            from ..models.hip_int8 import HipDeepLabInt8
            from ..models.quant import calibrate
            # activation scales from the serving distribution: letterboxed synthetic camera
            # frames at the model resolution (calibration_frames), not generic noise images
            import copy
            xc = calibration_frames(self.H, self.W, n=4, seed=cfg.seed).to(self.device)
            scales = calibrate(copy.deepcopy(self.model).float().to(self.device), xc)
            del xc
            self._hip_model = HipDeepLabInt8(self.model, self.device, cfg, scales=scales)
        else:
            from ..models.hip_model import HipDeepLab
            self._hip_model = HipDeepLab(self.model, self.device, cfg)
        self.stream = torch.cuda.Stream(self.device) if self.is_cuda else None

    # ------------------------------------------------------------------ setup
    def _load_weights(self, path: str) -> None:
        if path.endswith(".safetensors"):
            from safetensors.torch import load_file
            sd = load_file(path)
        else:
            sd = torch.load(path, map_location="cpu", weights_only=True)
        missing, unexpected = self.model.load_state_dict(sd, strict=False)
        log.info("loaded %s (missing=%d unexpected=%d)", path, len(missing), len(unexpected))

    def set_camera(self, cam_w: int, cam_h: int) -> None:
        if self.cam == (cam_w, cam_h):
            return
        self.cam = (int(cam_w), int(cam_h))
        lx, ly, rw, rh, cw, ch = R.letterbox_luts(cam_w, cam_h, self.W, self.H,
                                                  self.cfg.keep_aspect_ratio)
        self.crop_w, self.crop_h = cw, ch
        self.lut_x = torch.tensor(lx, device=self.device, dtype=torch.int32)
        self.lut_y = torch.tensor(ly, device=self.device, dtype=torch.int32)
        self._static_step = None  # captured for the previous camera's letterbox,
        self._bound_graphs = {}  # like the bound buffers' steps
        if self.zone_rows > 1:  # the zones of this camera's crop, in exact integers on the host
            from ..postprocess import zones as ZN
            self.zone_plane = ZN.rasterize(self.zone_list, cw, ch)
            if self._hip_post is not None:
                self._hip_post.set_zone_plane(self.zone_plane)

    # -------------------------------------------------------------- inference
    def to_bgr(self, frames: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The BGR frames of ``frames`` as ingested: themselves with ``pixel_format`` bgr;
        else their BT.601 conversion -- the gfx950 kernel on the HIP backend (into ``out``,
        a captured step's own buffer, if given), the torch definition otherwise."""
        if self.frame_channels == 3:
            return frames
        if frames.dim() != 4 or frames.shape[-1] != 2:
            raise ValueError(f"pixel_format {self.pixel_format}: frames must be (B, Hc, Wc, 2), "
                             f"got {tuple(frames.shape)}")
        uyvy = self.pixel_format == "uyvy"
        if self.backend == "hip":
            from ..ops import hip_ops
            return hip_ops.yuv422_to_bgr(frames, self.bgr_buffer(frames) if out is None else out, uyvy=uyvy)
        bgr = R.yuv422_to_bgr(frames, uyvy=uyvy)
        return bgr if out is None else out.copy_(bgr)

    def bgr_buffer(self, frames: torch.Tensor) -> Optional[torch.Tensor]:
        """A captured step's own BGR buffer for ``frames`` (None with ``pixel_format`` bgr)."""
        if self.frame_channels == 3:
            return None
        return torch.empty(tuple(frames.shape[:3]) + (3,), dtype=torch.uint8, device=frames.device)

    def _host_bgr(self, frame: np.ndarray) -> np.ndarray:
        """One host frame as BGR (the debug dump's image), by the host conversion."""
        if self.frame_channels == 3:
            return frame
        from ..ops.native import host
        h, w = frame.shape[:2]
        return host().yuv422_to_bgr(np.ascontiguousarray(frame).reshape(h, 2 * w),
                                    self.pixel_format == "uyvy")

    def _infer_eager(self, frames: torch.Tensor, bgr: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Label maps of frames as ingested; ``bgr``: where a raw format's BGR frames go."""
        frames = self.to_bgr(frames, out=bgr)
        if self.backend == "hip":
            return self._hip_model.segment(frames, self.lut_x, self.lut_y)
        x = R.preprocess(frames, self.lut_x, self.lut_y,
                         out_dtype=self.dtype, channels_last=self.is_cuda)
        with torch.no_grad():
            logits = self.model(x)
        return R.upsample_argmax(logits, self.H, self.W)

    def _infer(self, frames: torch.Tensor, bgr: Optional[torch.Tensor] = None):
        """(label maps, confidence plane) of frames as ingested; without ``serve_confidence``
        the label maps of ``_infer_eager`` and None."""
        if not self.serve_confidence:
            return (self._infer_eager(frames) if bgr is None else self._infer_eager(frames, bgr)), None
        frames = self.to_bgr(frames, out=bgr)
        if self.backend == "hip":
            labels = self._hip_model.segment(frames, self.lut_x, self.lut_y)
            B, Hc, Wc, _ = frames.shape
            return labels, self._hip_model.buffers(B, Hc, Wc)["conf"]
        x = R.preprocess(frames, self.lut_x, self.lut_y,
                         out_dtype=self.dtype, channels_last=self.is_cuda)
        with torch.no_grad():
            logits = self.model(x)
        return R.upsample_confidence(logits, self.H, self.W)

    def _device_post(self, labels: torch.Tensor, out: Optional[torch.Tensor] = None,
                     mask_out: Optional[torch.Tensor] = None,
                     region_out: Optional[torch.Tensor] = None,
                     conf: Optional[torch.Tensor] = None,
                     zone_out: Optional[torch.Tensor] = None,
                     presence_out: Optional[torch.Tensor] = None,
                     event_out: Optional[torch.Tensor] = None) -> torch.Tensor:
        return self._post_and_mask(labels, out, mask_out, region_out, conf, zone_out,
                                   presence_out, event_out)[0]  # the records alone

    def _post_and_mask(self, labels: torch.Tensor, out: Optional[torch.Tensor] = None,
                       mask_out: Optional[torch.Tensor] = None,
                       region_out: Optional[torch.Tensor] = None,
                       conf: Optional[torch.Tensor] = None,
                       zone_out: Optional[torch.Tensor] = None,
                       presence_out: Optional[torch.Tensor] = None,
                       event_out: Optional[torch.Tensor] = None):
        """(device records of ``labels``, with ``mask_cap`` their run-length masks else None,
        with ``region_cap`` their class regions else None), each right after the other on the
        same stream: one captured graph, a chain, holds all. ``conf``: the confidence plane of
        ``labels`` (``serve_confidence``), summed per region. With ``zone_rows`` the zone
        occupancy ends the chain; its words are ``device_zones()``. With ``presence_rows`` the
        zone presence follows it; its words are ``device_presence()``. With ``event_cap`` the zone
        events end the chain; their words are ``device_events()``."""
        if self._hip_post is None:
            from ..postprocess.device import DevicePostprocess
            # one histogram bin per model class (argmax labels are < num_classes): the
            # per-root fill histograms are the largest part of the workspace
            self._hip_post = DevicePostprocess(self.device, self.H, self.W, self.palette,
                                               self.cfg.max_segments,
                                               bins=max(1, min(256, self.cfg.num_classes)),
                                               mask_cap=self.mask_cap, region_cap=self.region_cap,
                                               region_classes=self.region_mask,
                                               region_min_pixels=self.region_min_pixels,
                                               region_conf=self.serve_confidence,
                                               track_streams=self.track_streams, track_q=self.track_q,
                                               zone_rows=self.zone_rows, zone_classes=self.zone_classes,
                                               zone_conf=self.zone_conf,
                                               presence_rows=self.presence_rows,
                                               presence_q=self.presence_q,
                                               stable_frames=self.stable_frames,
                                               stable_gate=self.stable_gate,
                                               stable_streams=self.stable_streams,
                                               **({"event_cap": self.event_cap} if self.event_cap else {}),
                                               **({"smooth_radius": self.smooth_radius}
                                                  if self.smooth_radius else {}))
            if self.zone_rows > 1:
                self._hip_post.set_zone_plane(self.zone_plane)
        kw = {"zone_out": zone_out} if self.zone_rows else {}
        if self.presence_rows:
            kw["presence_out"] = presence_out
        if self.event_cap:
            kw["event_out"] = event_out
        rec = self._hip_post.run(labels, self.crop_w, self.crop_h, self.min_area, out=out,
                                 mask_out=mask_out, region_out=region_out, conf=conf, **kw)
        return (rec, self._hip_post.last_mask if self.mask_cap else None,
                self._hip_post.last_regions if self.region_cap else None)

    def device_zones(self) -> Optional[torch.Tensor]:
        """The zone words the device post-processing wrote last (None without ``zone_rows``)."""
        return self._hip_post.last_zones if self.zone_rows and self._hip_post is not None else None

    def device_presence(self) -> Optional[torch.Tensor]:
        """The presence words the device post-processing wrote last (None without
        ``presence_rows``)."""
        return self._hip_post.last_presence if self.presence_rows and self._hip_post is not None else None

    def device_events(self) -> Optional[torch.Tensor]:
        """The event words the device post-processing wrote last (None without ``event_cap``)."""
        return self._hip_post.last_events if self.event_cap and self._hip_post is not None else None

    def _use_device_post(self) -> bool:
        return self.is_cuda and self.cfg.contour_mode == "fast"

    def host_masks(self, labels) -> np.ndarray:
        """uint32 [B, 4 + cap] run words of host label maps by the numpy definition
        (postprocess/mask_rle.py): the CPU path, and a GPU without device post-processing."""
        from ..postprocess import mask_rle as MR
        lab = labels.cpu().numpy() if isinstance(labels, torch.Tensor) else np.asarray(labels)
        out = np.zeros((lab.shape[0], 4 + self.mask_cap), np.uint32)
        for b in range(lab.shape[0]):
            MR.encode(lab[b], self.crop_w, self.crop_h, self.mask_cap, out=out[b])
        return out

    def track_layout(self, B: int) -> List[int]:
        """With ``track_regions`` or ``stable_frames``: the position (0 .. streams - 1) of the
        stream that owns each row of a batch of B frames -- consecutive rows per stream,
        feeder.split_batch."""
        from .feeder import split_batch
        n_streams = self.track_streams or self.stable_streams
        return [s for s, n in enumerate(split_batch(B, n_streams)) for _ in range(n)]

    def check_track_streams(self, streams, B: int) -> None:
        """With ``track_regions`` or ``stable_frames`` on the device: raise unless the
        ``streams`` of a batch follow the layout the stateful kernels were built for, with the
        same stream ids as before."""
        if not (self.track_regions or self.stable_frames):
            return
        got, want = _per_frame(streams, B), self.track_layout(B)
        ids = dict(self._track_ids)
        ok = len(got) == B and all(ids.setdefault(pos, st) == st for pos, st in zip(want, got))
        if not ok or len(set(ids.values())) != len(ids):
            flag = "--track_regions" if self.track_regions else "--stable_labels"
            raise ValueError(f"{flag}: the streams {got} of a batch of {B} frames do not follow "
                             f"the layout {want} of --streams {self.track_streams or self.stable_streams} "
                             f"(consecutive rows per stream, the same streams every step; so far "
                             f"{self._track_ids})")
        self._track_ids = ids

    def reset_tracks(self) -> None:
        """Forget the tracks of every stream: the next frame's regions are all new, from id 1;
        with ``stable_frames`` forget the stabilisation state too: the next frame's labels pass
        unchanged. Called after warm-up and capture (their steps advance the state) and when a
        producer or pipeline starts. Waits for the device."""
        if not (self.track_regions or self.stable_frames):
            return
        if self._trackers is not None:
            self._trackers.reset()
        if self._stabilizers is not None:
            self._stabilizers.reset()
        self._track_ids = {}
        if self._dwells is not None:
            self._dwells.reset()
        if self._events is not None:
            self._events.reset()
        if self._hip_post is not None:
            self._hip_post.reset_tracks()

    def host_smooth(self, labels: torch.Tensor, conf: Optional[torch.Tensor]):
        """``smooth_radius`` on the host paths (the CPU, and a GPU without device
        post-processing), ahead of ``host_stable``: ``labels`` (and ``conf``) are overwritten in
        place with the smoothed planes (postprocess/smooth.py), which are also returned."""
        from ..postprocess import smooth as SM
        lab, cf = SM.apply(labels.cpu().numpy(), None if conf is None else conf.cpu().numpy(),
                           self.crop_w, self.crop_h, self.smooth_radius)
        labels.copy_(torch.from_numpy(lab))
        if conf is not None:
            conf.copy_(torch.from_numpy(cf))
        return labels, conf

    def host_stable(self, labels: torch.Tensor, conf: Optional[torch.Tensor], streams=None):
        """``stable_frames`` on the host paths (the CPU, and a GPU without device
        post-processing): the frames advance the StreamStabilizer of their ``streams`` (default:
        the layout positions of ``track_layout``) in row order, and ``labels`` (and ``conf``) are
        overwritten in place with the stabilised planes, which are also returned."""
        B = labels.shape[0]
        streams = self.track_layout(B) if streams is None else _per_frame(streams, B)
        lab, cf = self._stabilizers.step(labels.cpu().numpy(), None if conf is None else conf.cpu().numpy(),
                                         self.crop_w, self.crop_h, streams)
        labels.copy_(torch.from_numpy(lab))
        if conf is not None:
            conf.copy_(torch.from_numpy(cf))
        return labels, conf

    def host_regions(self, labels, conf=None, streams=None) -> np.ndarray:
        """uint32 [B, 4 + 6 cap] region words of host label maps by the numpy definition
        (postprocess/regions.py): the CPU path, and a GPU without device post-processing. With
        ``serve_confidence``, ``conf`` is their confidence plane and the rows are [B, 4 + 7 cap].
        With ``track_regions`` two more words a record: the frames advance the StreamTracker of
        their ``streams`` (default: the layout positions of ``track_layout``), in row order."""
        from ..postprocess import regions as RG
        lab = labels.cpu().numpy() if isinstance(labels, torch.Tensor) else np.asarray(labels)
        kw = [{}] * lab.shape[0]
        if self.track_regions:
            streams = self.track_layout(lab.shape[0]) if streams is None else _per_frame(streams, lab.shape[0])
            kw = [{"tracker": self._trackers.of(s)} for s in streams]
        if self.serve_confidence:
            if conf is None:
                raise ValueError("host_regions: serve_confidence needs the conf plane")
            conf = conf.cpu().numpy() if isinstance(conf, torch.Tensor) else np.asarray(conf)
        else:
            conf = None
        out = np.zeros((lab.shape[0], 4 + self.region_words * self.region_cap), np.uint32)
        for b in range(lab.shape[0]):
            RG.encode(lab[b], self.crop_w, self.crop_h, self.region_mask, self.region_min_pixels,
                      self.region_cap, out=out[b], conf=None if conf is None else conf[b], **kw[b])
        return out

    def host_zones(self, labels, conf=None) -> np.ndarray:
        """uint32 [B, 4 + R C] zone words of host label maps by the numpy definition
        (postprocess/zones.py): the CPU path, and a GPU without device post-processing. With
        ``serve_confidence``, ``conf`` is their confidence plane and the rows are [B, 4 + 2 R C]."""
        from ..postprocess import zones as ZN
        lab = labels.cpu().numpy() if isinstance(labels, torch.Tensor) else np.asarray(labels)
        if self.zone_conf:
            if conf is None:
                raise ValueError("host_zones: serve_confidence needs the conf plane")
            conf = conf.cpu().numpy() if isinstance(conf, torch.Tensor) else np.asarray(conf)
        else:
            conf = None
        out = np.zeros((lab.shape[0], ZN.frame_words(self.zone_rows, self.zone_classes, self.zone_conf)),
                       np.uint32)
        for b in range(lab.shape[0]):
            ZN.encode(lab[b], self.zone_plane, self.crop_w, self.crop_h, self.zone_classes,
                      conf=None if conf is None else conf[b], out=out[b], rows=self.zone_rows)
        return out

    def host_presence(self, labels, regions, streams=None) -> np.ndarray:
        """uint32 [B, 4 + U cap] presence words of host label maps by the numpy definition
        (postprocess/presence.py): the CPU path, and a GPU without device post-processing.
        ``regions``: the region words of the same frames (``host_regions``: with ``track_regions``
        their track ids and ages are read, and the frames advance the StreamDwell of their
        ``streams``, as there)."""
        from ..postprocess import presence as PR
        from ..postprocess import regions as RG
        lab = labels.cpu().numpy() if isinstance(labels, torch.Tensor) else np.asarray(labels)
        reg = regions.cpu().numpy() if isinstance(regions, torch.Tensor) else np.asarray(regions)
        tr = self.presence_tracks
        if tr:
            streams = self.track_layout(lab.shape[0]) if streams is None else _per_frame(streams, lab.shape[0])
        out = np.zeros((lab.shape[0], PR.frame_words(self.region_cap, self.presence_rows, tr)), np.uint32)
        for b in range(lab.shape[0]):
            tab = RG.decode(reg[b], conf=self.serve_confidence, tracks=True) if tr else None
            PR.encode(lab[b], self.zone_plane, self.crop_w, self.crop_h, self.region_mask,
                      self.region_min_pixels, self.region_cap, self.presence_rows, self.presence_q,
                      tab=tab, dwell=self._dwells.of(streams[b]) if tr else None, out=out[b])
        return out

    def host_events(self, presence, streams=None) -> np.ndarray:
        """uint32 [B, 4 + 4 E] event words of host presence words by the numpy definition
        (postprocess/events.py): the CPU path, and a GPU without device post-processing.
        ``presence``: the presence words of the frames (``host_presence``); the frames advance the
        StreamEvents of their ``streams`` in row order, as the dwell state there."""
        from ..postprocess import events as EV
        from ..postprocess import presence as PR
        pr = presence.cpu().numpy() if isinstance(presence, torch.Tensor) else np.asarray(presence)
        pr = pr.view(np.uint32)
        streams = self.track_layout(pr.shape[0]) if streams is None else _per_frame(streams, pr.shape[0])
        out = np.zeros((pr.shape[0], EV.frame_words(self.event_cap)), np.uint32)
        for b in range(pr.shape[0]):
            self._events.of(streams[b]).update(PR.decode(pr[b], self.presence_rows, tracks=True), out=out[b])
        return out

    def _step_outputs(self, frames: torch.Tensor, bgr: Optional[torch.Tensor] = None):
        """One eager step: (labels, packed records or None, mask run words or None, region
        words or None)."""
        return self._step_all(frames, bgr)[:4]

    def _step_all(self, frames: torch.Tensor, bgr: Optional[torch.Tensor] = None):
        """``_step_outputs`` and, fifth, the confidence plane (None without ``serve_confidence``)."""
        labels, conf = self._infer(frames, bgr)
        if self._use_device_post():
            out = (labels, *self._post_and_mask(labels, conf=conf), conf)
            self._step_zones = self.device_zones()
            self._step_presence = self.device_presence()
            self._step_events = self.device_events()
            return out
        # no device post-processing: on the CPU the masks are encoded here; a GPU's host
        # post-processing path encodes them where it brings the label maps to the host
        host = not self.is_cuda
        if host and self.smooth_radius:  # a GPU's host path: run_device, once the maps exist
            labels, conf = self.host_smooth(labels, conf)
        if host and self.stable_frames:  # the same
            labels, conf = self.host_stable(labels, conf)
        mask = torch.from_numpy(self.host_masks(labels).view(np.int32)) if host and self.mask_cap else None
        regions = torch.from_numpy(self.host_regions(labels, conf).view(np.int32)) \
            if host and self.region_cap else None
        self._step_zones = torch.from_numpy(self.host_zones(labels, conf).view(np.int32)) \
            if host and self.zone_rows else None
        self._step_presence = torch.from_numpy(self.host_presence(labels, regions).view(np.int32)) \
            if host and self.presence_rows else None
        self._step_events = torch.from_numpy(self.host_events(self._step_presence).view(np.int32)) \
            if host and self.event_cap else None
        post = self._host_packed(labels) if host and self.cfg.contour_mode != "none" else None
        return labels, post, mask, regions, conf

    def _step_device(self, frames: torch.Tensor):
        labels, post, self.mask_packed, self.region_packed, self.conf_plane = self._step_all(frames)
        self.zone_packed = self._step_zones
        self.presence_packed = self._step_presence
        self.events_packed = self._step_events
        return labels, post

    def _host_packed(self, labels: torch.Tensor) -> torch.Tensor:
        """CPU path: host post-processing packed like the device output
        ([B, 1 + 5K] float32: count, then (label, score, area, cx, cy) per record),
        so the data-parallel gather is identical on CPU (gloo) and GPU (RCCL)."""
        K = self.cfg.max_segments
        B = labels.shape[0]
        recs = self.records_from_labels(labels, [0] * B, [0.0] * B, list(range(B)))
        out = torch.zeros((B, 1 + 5 * K), dtype=torch.float32)
        for b in range(B):
            r = recs[recs["stream"] == b][:K]
            out[b, 0] = len(r)
            if len(r):
                vals = np.stack([r["label"].astype(np.float32), r["score"], r["area"], r["cx"], r["cy"]], 1)
                out[b, 1:1 + 5 * len(r)] = torch.from_numpy(vals.reshape(-1))
        return out

    @property
    def _static(self) -> Dict[str, torch.Tensor]:
        """The static step's frames, labels, post, mask (empty before the first static run)."""
        return vars(self._static_step) if self._static_step is not None else {}

    def bind_inputs(self, bufs, split_post: bool = False) -> None:
        """Declare persistent frame buffers (e.g. the DP pipeline's double-buffered
        staging slots): ``run_device`` on one of them replays a graph captured with
        that buffer as its input, so the step reads the frames in place instead of
        copying them into the single static input first (one D2D copy of
        B x Hc x Wc x 3 bytes and one launch per step saved).

        ``split_post``: per slot, TWO graphs -- the model (frames -> the slot's own
        label maps) on the caller's stream and the device post-processing (labels
        -> packed records) on ``result_stream``. The post-processing kernels are
        latency-bound (union-find chains, per-frame merges, few workgroups), so step
        k's post-processing runs concurrently with step k+1's model instead of
        idling the chip at the end of every step. Consumers of the packed records
        must be ordered after ``result_stream`` (the DP pipeline enqueues its gather
        and D2H copy there)."""
        if not (self.cfg.graph and self.is_cuda):
            return
        self._split = bool(split_post) and self._use_device_post()
        self.result_stream = torch.cuda.Stream(self.device) if self._split else None
        # SSA_MODEL_PARTS=P: the model of each step as P concurrent sub-batch graphs on P
        # streams, each followed by its own post-processing graph (split_post path; B % P
        # == 0 and B >= 2P, else one graph). Measured at B = 32: 2 parts 26.0k frames/s vs
        # 24.0k for one graph (profiles/r2_parts_ab.txt); slot-parallel (default, below)
        # measured faster still, so parts are off unless asked for.
        self.model_parts = int(os.environ.get("SSA_MODEL_PARTS", "1"))
        if self.track_regions and self.model_parts > 1:
            raise ValueError("--track_regions is not supported with SSA_MODEL_PARTS > 1: the parts of "
                             "a batch are post-processed separately, not as one batch in stream order")
        if self.stable_frames and self.model_parts > 1:
            raise ValueError("--stable_labels is not supported with SSA_MODEL_PARTS > 1: the parts of "
                             "a batch are post-processed separately, not as one batch in stream order")
        self.model_streams = []
        self._bound = {b.data_ptr(): b for b in bufs}
        self._slot_of = {b.data_ptr(): i for i, b in enumerate(bufs)}
        # slot-parallel (default; SSA_SLOT_PARALLEL=0 turns it off): every staging slot owns
        # a plan copy and a model stream, so step k+1's model runs concurrently with step
        # k's. Latency-bound kernels of one step fill the other's tails: B = 32 26.9k /
        # 27.3k frames/s vs 25.9k / 25.6k for 2 sub-batch parts, batch 1 0.39 / 0.38 ms per
        # frame vs 0.52 / 0.48 (profiles/r2_slot_ab.txt). Round 2 kept it opt-in because
        # concurrent plan copies gave rare label-map mismatches; round 3 traced those to
        # packed-f32 VALU results corrupted under co-residence (profiles/r3_packed_f32_race.txt)
        # and builds without them: 0 / 900 and 0 / 300 (headline shape) concurrent mismatches.
        # (needs plan copies: the bf16 and int8 HIP models (models/plan.py); the torch path
        # has no plan, so its slots stay on the caller's stream)
        self.slot_parallel = (os.environ.get("SSA_SLOT_PARALLEL", "1") == "1" and self._split
                              and self._hip_model is not None)
        self.last_consumed = None
        # uploads on the slot streams (default; SSA_H2D_ON_SLOT=0: a copy stream): the
        # pipeline uploads a slot's frames on that slot's model stream, in order before its
        # model, so no copy stream and no fork from the caller's stream -- 3 active streams
        # (2 slots + result) on the 4 hardware queues. B = 32 28.0k / 28.1k vs 27.5k / 26.9k
        # frames/s; batch 1 0.340 / 0.356 vs 0.381 / 0.379 ms (profiles/r2_h2d_ab.txt)
        self.h2d_on_slot = self.slot_parallel and os.environ.get("SSA_H2D_ON_SLOT", "1") == "1"
        self.slot_streams = [torch.cuda.Stream(self.device) for _ in bufs] if self.slot_parallel else []
        self._bound_graphs = {}
        if self.cam is not None:  # capture now, not inside the first timed steps
            for b in bufs:
                self._bound_step(b)

    def _bound_step(self, frames: torch.Tensor):
        """The captured step of a buffer declared with ``bind_inputs`` (None: not one)."""
        key = frames.data_ptr()
        b = self._bound.get(key)
        if b is None or b.shape != frames.shape or b.dtype != frames.dtype:
            return None
        step = self._bound_graphs.get(key)
        if step is None:
            step = self._bound_graphs[key] = capture(self, b, slot=self._slot_of[key])
            self.reset_tracks()  # the warm-up steps of the capture advanced them
        return step

    def preferred_lag(self) -> int:
        """Pipeline lag this engine runs best at: 2 (three staging slots, three steps in
        flight) when it will run slot-parallel with uploads on the slot streams -- 3 slot
        streams + the result stream fit the 4 hardware queues. Measured: B = 32 30.9k /
        29.2k vs 28.3k / 28.0k frames/s at lag 1; batch 1 0.236 vs 0.351 ms per frame
        (profiles/r2_lag_ab.txt). Otherwise 1."""
        ok = (self.is_cuda and self.cfg.graph and self._use_device_post()
              and self._hip_model is not None
              and os.environ.get("SSA_SPLIT_POST", "1") != "0"
              and os.environ.get("SSA_SLOT_PARALLEL", "1") == "1"
              and os.environ.get("SSA_H2D_ON_SLOT", "1") == "1")
        return 2 if ok else 1

    def upload_stream(self, buf: torch.Tensor):
        """Stream to upload a bound staging slot's frames on (SSA_H2D_ON_SLOT), else None."""
        if not self.h2d_on_slot:
            return None
        i = self._slot_of.get(buf.data_ptr())
        return None if i is None else self.slot_streams[i]

    def run_device(self, frames: torch.Tensor):
        """frames: (B, Hc, Wc, 3) uint8 on this device (raw pixel formats: (B, Hc, Wc, 2))
        -> (labels, device post outputs).

        With ``cfg.graph`` the step is captured on first use per (B, camera) and
        replayed; outputs then live in static buffers overwritten by the next call.
        Frames in a buffer declared with ``bind_inputs`` run that buffer's own graph
        (with ``split_post``, the records are produced on ``result_stream``).
        """
        if not (self.cfg.graph and self.is_cuda):
            labels, post = self._step_device(frames)
            return self._gpu_host_stable(labels), post
        step = self._bound_step(frames)
        if step is None:  # the engine's own static input buffer, for this batch size
            step, B = self._static_step, frames.shape[0]
            if step is None or step.frames.shape[0] != B:
                buf = torch.zeros((B, self.cam[1], self.cam[0], self.frame_channels), dtype=torch.uint8,
                                  device=self.device)
                step = self._static_step = capture(self, buf)
                self.reset_tracks()  # the warm-up steps of the capture advanced them
            step.frames.copy_(frames, non_blocking=True)
        step.replay()
        # written by the replay, like the records; and when the frame buffer may be refilled
        self.mask_packed, self.region_packed, self.last_consumed = step.mask, step.regions, step.consumed
        self.conf_plane = step.conf
        self.zone_packed = step.zones
        self.presence_packed = step.presence
        self.events_packed = getattr(step, "events", None)
        return self._gpu_host_stable(step.labels), step.post

    def _gpu_host_stable(self, labels: torch.Tensor) -> torch.Tensor:
        """``smooth_radius`` and ``stable_frames`` on a GPU without device post-processing: the
        label maps (and ``conf_plane``) of the step just issued are smoothed, then stabilised, on
        the host and written back in place, once the stream has produced them; every consumer
        then reads those. Anything else: ``labels`` as they are (the device chain has cleaned
        them already)."""
        if (self.smooth_radius or self.stable_frames) and self.is_cuda and not self._use_device_post():
            torch.cuda.current_stream(self.device).synchronize()
            if self.smooth_radius:
                self.host_smooth(labels, self.conf_plane)
            if self.stable_frames:
                self.host_stable(labels, self.conf_plane)
        return labels

    # ------------------------------------------------------------ post/host
    def records_from_labels(self, labels: torch.Tensor, frame_ids: Sequence[int],
                            ts: Sequence[float], streams) -> np.ndarray:
        """Host post-processing of label maps (exact tracer, or CPU component path)."""
        if self.cfg.contour_mode == "none":  # ablation: inference only
            return np.zeros(0, RECORD_DTYPE)
        lab = labels.cpu().numpy() if labels.device.type != "cpu" else labels.numpy()
        streams = _per_frame(streams, lab.shape[0])
        out = []
        for i in range(lab.shape[0]):
            out.append(PR.frame_records(lab[i], self.crop_w, self.crop_h, self.cfg.min_area_ratio,
                                        self.palette, streams[i], frame_ids[i], ts[i])
                       if self.cfg.contour_mode == "exact" or not self._has_scipy()
                       else self._component_records(lab[i], streams[i], frame_ids[i], ts[i]))
        return np.concatenate(out) if out else np.zeros(0, RECORD_DTYPE)

    @staticmethod
    def _has_scipy() -> bool:
        try:
            import scipy.ndimage  # noqa: F401
            return True
        except Exception:
            return False

    def _component_records(self, lab: np.ndarray, stream: int, fid: int, ts: float) -> np.ndarray:
        from ..postprocess.components import component_segments
        segs = component_segments(lab[: self.crop_h, : self.crop_w], self.min_area, self.palette)
        out = np.zeros(len(segs), RECORD_DTYPE)
        H, W = self.H, self.W
        for i, (l, sc, area, cx, cy, _, _) in enumerate(segs):
            out[i] = (l, sc, min(1.0, area / (W * H)), min(1.0, cx / W), min(1.0, cy / H),
                      stream, fid, ts)
        return out

    def step(self, frames_host: np.ndarray, frame_ids: Sequence[int], ts: Sequence[float],
             streams=0) -> np.ndarray:
        """Full step from host frames ((B, Hc, Wc, 3) BGR; raw pixel formats: (B, Hc, Wc, 2)
        packed bytes) to records (used by the server producer)."""
        if frames_host.ndim != 4 or frames_host.shape[-1] != self.frame_channels:
            raise ValueError(f"pixel_format {self.pixel_format}: frames must be (B, Hc, Wc, "
                             f"{self.frame_channels}), got {tuple(frames_host.shape)}")
        Hc, Wc = frames_host.shape[1:3]
        self.set_camera(Wc, Hc)
        if not self.is_cuda:
            frames = torch.from_numpy(np.ascontiguousarray(frames_host))
            with torch.no_grad():
                labels, self.conf_plane = self._infer(frames)
            if self.smooth_radius:
                labels, self.conf_plane = self.host_smooth(labels, self.conf_plane)
            if self.stable_frames:
                labels, self.conf_plane = self.host_stable(labels, self.conf_plane,
                                                           _per_frame(streams, len(frame_ids)))
            if self.debug is not None and self.debug.want():
                self.debug.dump(self._host_bgr(frames_host[0]), labels[0].numpy(), self.crop_w, self.crop_h,
                                _per_frame(streams, len(frame_ids))[0], int(frame_ids[0]))
            if self.mask_cap:
                self.masks = self.host_masks(labels)
            if self.region_cap:
                self.regions = self.host_regions(labels, self.conf_plane, streams)
            if self.zone_rows:
                self.zones = self.host_zones(labels, self.conf_plane)
            if self.presence_rows:
                self.presence = self.host_presence(labels, self.regions, streams)
            if self.event_cap:
                self.events = self.host_events(self.presence, streams)
            return self.records_from_labels(labels, frame_ids, ts, streams)
        tr = self.tracer
        if self._use_device_post():
            self.check_track_streams(streams, len(frame_ids))
        with torch.cuda.stream(self.stream):
            with tr.stage("h2d", self.stream):
                frames = torch.from_numpy(np.ascontiguousarray(frames_host)).pin_memory() \
                    .to(self.device, non_blocking=True)
            with tr.stage("model+post", self.stream):
                labels, post = self.run_device(frames)
            if post is not None:
                with tr.stage("d2h+records", self.stream):
                    recs = self._hip_post.fetch(post, frame_ids, ts,
                                                _per_frame(streams, len(frame_ids)), self.W, self.H)
                if self.mask_cap:  # same stream, after the records: one more small D2H
                    self.masks = self._hip_post.fetch_masks(self.mask_packed)
                if self.region_cap:
                    self.regions = self._hip_post.fetch_regions(self.region_packed)
                if self.zone_rows:
                    self.zones = self._hip_post.fetch_zones(self.zone_packed)
                if self.presence_rows:
                    self.presence = self._hip_post.fetch_presence(self.presence_packed)
                if self.event_cap:
                    self.events = self._hip_post.fetch_events(self.events_packed)
            else:
                recs = None
        self.stream.synchronize()
        if self.mask_cap and post is None:
            self.masks = self.host_masks(labels)
        if self.region_cap and post is None:
            self.regions = self.host_regions(labels, self.conf_plane, streams)
        if self.zone_rows and post is None:
            self.zones = self.host_zones(labels, self.conf_plane)
        if self.presence_rows and post is None:
            self.presence = self.host_presence(labels, self.regions, streams)
        if self.event_cap and post is None:
            self.events = self.host_events(self.presence, streams)
        if self.debug is not None and self.debug.want():
            self.debug.dump(self._host_bgr(frames_host[0]), labels[0].cpu().numpy(), self.crop_w, self.crop_h,
                            _per_frame(streams, len(frame_ids))[0], int(frame_ids[0]))
        if recs is None:
            with tr.stage("host_post"):
                recs = self.records_from_labels(labels, frame_ids, ts, streams)
        return recs
