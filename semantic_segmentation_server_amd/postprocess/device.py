"""Device-side contour statistics (HIP kernels in ``csrc/hip/postprocess.hip``).

Static workspace + packed output per batch size so the whole thing replays
inside the engine's hipGraph; ``fetch`` does the single small D2H copy of the
packed records (1 + 5K floats per frame) and unpacks them in push order.
"""
from __future__ import annotations

import os

from typing import Dict, Sequence

import numpy as np
import torch

from ..ops import hip_ops
from ..runtime.results import RECORD_DTYPE


class DevicePostprocess:
    def __init__(self, device: torch.device, H: int, W: int, palette: np.ndarray, K: int = 64,
                 bins: int = 32, thr: int = 127, mask_cap: int = 0, region_cap: int = 0,
                 region_classes: int = 0, region_min_pixels: int = 1, region_conf: bool = False,
                 track_streams: int = 0, track_q: int = 0, zone_rows: int = 0, zone_classes: int = 0,
                 zone_conf: bool = False, presence_rows: int = 0, presence_q: int = 0,
                 stable_frames: int = 0, stable_gate: int = 0, stable_streams: int = 0,
                 event_cap: int = 0, smooth_radius: int = 0):
        self.device = device
        # smooth_radius (--smooth_labels): R of the windowed majority filter (label_smooth.hip),
        # the first launch of run(), ahead of the stabilisation: out of place into a scratch
        # plane per batch size (and a scratch code plane when a confidence plane is passed),
        # from which the stabilisation writes the caller's planes, or a copy on the same stream
        # without it -- either way the caller's planes hold the cleaned maps and every later
        # kernel reads those. Stateless. 0: no kernel, no buffer, no launch
        self.smooth_radius = int(smooth_radius)
        if self.smooth_radius:
            from . import smooth as SM
            SM.check_params(self.smooth_radius)
        self._smooth_bufs: Dict[tuple, tuple] = {}
        # event_cap (--serve_events): E of the zone-event kernels (zone_events.hip), the events
        # stored per frame; 0: no kernel, no buffer, no launch. They end the chain, read the
        # presence rows of the run and the track layout, and carry per stream its last presence
        # row beside the dwell state (reset_tracks clears it too)
        self.event_cap = int(event_cap)
        if self.event_cap and not (presence_rows and track_streams):
            raise ValueError("DevicePostprocess: event_cap needs presence_rows and track_streams")
        self._event_bufs: Dict[tuple, torch.Tensor] = {}
        self._event_state: Dict[tuple, torch.Tensor] = {}
        self.last_events = None
        # stable_frames (--stable_labels): N of the temporal label stabilisation
        # (label_stable.hip), the first launch of run(): in place on the label maps (and on the
        # confidence plane when one is passed), so every later kernel reads the stabilised
        # planes. 0: no kernel, no buffer, no launch. stable_gate: the gate code of
        # --stable_min_confidence. stable_streams: the streams whose frames this object sees,
        # laid out like track_streams (and equal to it when both are on); their carried state
        # lives beside the track state (reset_tracks clears it too)
        self.stable_frames, self.stable_gate = int(stable_frames), int(stable_gate)
        self.stable_streams = int(stable_streams)
        if self.stable_frames:
            from . import stable as SB
            SB.check_params(self.stable_frames, self.stable_gate, True)
            if self.stable_streams < 1:
                raise ValueError("DevicePostprocess: stable_frames needs stable_streams")
            if track_streams and int(track_streams) != self.stable_streams:
                raise ValueError("DevicePostprocess: stable_streams differs from track_streams")
        self._stable_tables: Dict[int, torch.Tensor] = {}
        self._stable_state: Dict[tuple, torch.Tensor] = {}
        # presence_rows (--serve_presence): R of the zone-presence kernels (zone_presence.hip),
        # the zone rows; 0: no kernel, no buffer, no launch. They follow the region (and track)
        # and zone kernels, read the zone plane of the crop, and with track_streams carry a
        # dwell state per stream beside the track state (reset_tracks clears both)
        self.presence_rows, self.presence_q = int(presence_rows), int(presence_q)
        if self.presence_rows and not (region_cap and self.presence_rows == int(zone_rows)):
            raise ValueError("DevicePostprocess: presence_rows needs region_cap and equals zone_rows")
        self._presence_bufs: Dict[tuple, tuple] = {}
        self._presence_state: Dict[tuple, torch.Tensor] = {}
        self.last_presence = None
        # zone_rows (--serve_zones): R = 1 + the user zones of the zone-occupancy kernel
        # (zone_stats.hip), zone_classes its C; 0: no kernel, no buffer, no launch. zone_conf:
        # run() takes the confidence plane and the rows have the sum_conf block. The zone plane
        # (set_zone_plane) belongs to the crop and is shared by every batch size and every graph
        self.zone_rows, self.zone_classes = int(zone_rows), int(zone_classes)
        self.zone_conf = bool(zone_conf)
        if self.zone_rows and not self.zone_classes:
            raise ValueError("DevicePostprocess: zone_rows needs zone_classes")
        self._zone_bufs: Dict[tuple, tuple] = {}
        self._zone_plane: Dict[tuple, torch.Tensor] = {}
        self.last_zones = None
        # region_conf (--serve_confidence): run() takes the confidence plane beside the labels
        # and the region records have 7 words (sum_conf)
        self.region_conf = bool(region_conf)
        self.region_words = 7 if self.region_conf else 6
        # track_streams (--track_regions): the number of streams whose frames this object sees,
        # each batch of B frames laid out by feeder.split_batch(B, track_streams). The region
        # kernels then write their 6- / 7-word rows to a buffer of their own and the tracking
        # kernels (hip_ops.region_tracks) the served rows, two words wider. 0: no launch, no
        # buffer. The streams' carried state is shared by every batch size and every graph.
        self.track_streams, self.track_q = int(track_streams), int(track_q)
        if self.track_streams and not region_cap:
            raise ValueError("DevicePostprocess: track_streams needs region_cap")
        self.out_words = self.region_words + (2 if self.track_streams else 0)
        self._track_bufs: Dict[tuple, tuple] = {}
        self._track_state: Dict[tuple, torch.Tensor] = {}
        # records per frame of the class-region kernels (class_regions.hip); 0: no kernel, no
        # buffer, no launch. region_classes: the served 256-bit class set
        self.region_cap = int(region_cap)
        self.region_classes, self.region_min_pixels = int(region_classes), int(region_min_pixels)
        self._region_bufs: Dict[tuple, tuple] = {}
        self.last_regions = None
        # run slots per frame of the label-mask encoder (mask_rle.hip); 0: no encoder, no
        # buffer, no launch
        self.mask_cap = int(mask_cap)
        self._mask_bufs: Dict[tuple, tuple] = {}
        self.H, self.W, self.K, self.bins, self.thr = H, W, K, bins, thr
        self.palette = torch.tensor(np.asarray(palette, np.int32).reshape(256, 3), device=device)
        self._bufs: Dict[int, tuple] = {}
        self._host: Dict[int, torch.Tensor] = {}
        self._mask_host: Dict[int, torch.Tensor] = {}
        self.last_mask = None
        # accumulation pass: pixel strips (0), LDS-staged 32 x 32 (1) or 64 x 64 (2) tiles;
        # unset: by batch size (accum_for)
        env = os.environ.get("SSA_POST_ACCUM")
        self.accum = int(env) if env is not None else None

    def accum_for(self, B: int) -> int:
        """The accumulation pass for a batch of B frames: the LDS-staged 32 x 32 tiles at every
        batch size since round 5's slot tables (batch 1: 18.6 vs 20.5 us for round 3's strips,
        5678 vs 5456 frames/s, p50 0.625 vs 0.638 ms, profiles/r6b_b1_accum_ab.txt; batch 32:
        64.8 vs 219 us per 32 bench frames, r5t). More than 32 classes use the strips (the
        tile kernel's dense class counters hold 32)."""
        if self.accum is not None:
            return self.accum
        return 1
    def _buffers(self, B: int):
        if B not in self._bufs:
            nbytes = hip_ops.post_workspace_bytes(B, self.H, self.W, self.K, self.bins)
            ws = torch.zeros(nbytes, dtype=torch.uint8, device=self.device)  # deterministic start
            rec = torch.zeros((B, 1 + 5 * self.K), dtype=torch.float32, device=self.device)
            self._bufs[B] = (ws, rec)
        return self._bufs[B]

    def mask_buffers(self, B: int, crop_w: int, crop_h: int):
        """(workspace, [B, 4 + mask_cap] int32 run words) of the mask encoder for a batch of B
        frames: static like the records buffer, shared by every slot, ordered by the stream
        the post-processing runs on."""
        key = (B, crop_w, crop_h)
        if key not in self._mask_bufs:
            from . import mask_rle as MR
            MR.check_geometry(crop_w, crop_h, self.mask_cap)
            ws = torch.zeros(max(4, hip_ops.mask_rle_workspace_bytes(B, crop_h, crop_w)),
                             dtype=torch.uint8, device=self.device)
            words = torch.zeros((B, 4 + self.mask_cap), dtype=torch.int32, device=self.device)
            self._mask_bufs[key] = (ws, words)
        return self._mask_bufs[key]

    def region_buffers(self, B: int, crop_w: int, crop_h: int):
        """(workspace, [B, 4 + 6 region_cap] int32 region words) of the class-region kernels for
        a batch of B frames: static and shared like ``mask_buffers``. The kernels of every run
        initialise what they read of the workspace. With ``region_conf``: 7 words a region."""
        key = (B, crop_w, crop_h)
        if key not in self._region_bufs:
            from . import regions as RG
            RG.check_geometry(crop_w, crop_h, self.region_min_pixels, self.region_cap)
            ws = torch.zeros(hip_ops.class_regions_workspace_bytes(B, crop_h, crop_w, self.region_conf),
                             dtype=torch.uint8, device=self.device)
            words = torch.zeros((B, 4 + self.region_words * self.region_cap), dtype=torch.int32,
                                device=self.device)
            self._region_bufs[key] = (ws, words)
        return self._region_bufs[key]

    def zone_buffers(self, B: int, crop_w: int, crop_h: int):
        """(workspace, [B, 4 + R C] int32 zone words, [B, 4 + 2 R C] with ``zone_conf``) of the
        zone-occupancy kernel for a batch of B frames: static and shared like ``mask_buffers``.
        Every run writes every word."""
        key = (B, crop_w, crop_h)
        if key not in self._zone_bufs:
            from . import zones as ZN
            ZN.check_geometry(crop_w, crop_h, self.zone_rows - 1, self.zone_classes)
            ws = torch.zeros(hip_ops.zone_stats_workspace_bytes(B, self.zone_rows, self.zone_classes,
                                                                self.zone_conf),
                             dtype=torch.uint8, device=self.device)
            words = torch.zeros((B, ZN.frame_words(self.zone_rows, self.zone_classes, self.zone_conf)),
                                dtype=torch.int32, device=self.device)
            self._zone_bufs[key] = (ws, words)
        return self._zone_bufs[key]

    def set_zone_plane(self, plane: np.ndarray) -> None:
        """The rasterised zones of a crop (uint32 [crop_h, crop_w], postprocess/zones.py
        ``rasterize``), uploaded once; the runs of that crop read it. A plane already set for
        the crop is overwritten in place (captured graphs keep the address), once the device
        is idle."""
        if self.zone_rows < 2:
            raise ValueError("DevicePostprocess.set_zone_plane: no user zones (zone_rows < 2)")
        plane = np.ascontiguousarray(plane, np.uint32)
        if plane.ndim != 2:
            raise ValueError(f"zone plane: shape {plane.shape} is not (crop_h, crop_w)")
        if int(plane.max(initial=0)) >> (self.zone_rows - 1):
            raise ValueError(f"zone plane: bits past the {self.zone_rows - 1} user zones")
        key = (plane.shape[1], plane.shape[0])
        t = torch.from_numpy(plane.view(np.int32))
        if key in self._zone_plane:
            torch.cuda.synchronize(self.device)
            self._zone_plane[key].copy_(t)
            torch.cuda.synchronize(self.device)
        else:
            self._zone_plane[key] = t.to(self.device)

    def track_counts(self, B: int):
        """The rows of a batch of B frames that each stream owns (consecutive, in stream order)."""
        from ..runtime.feeder import split_batch
        return split_batch(B, self.track_streams or self.stable_streams)

    def smooth_buffers(self, B: int, conf: bool):
        """(scratch label plane, scratch code plane or None) of the label smoothing for a batch
        of B frames: static like the records buffer. Every run writes every byte."""
        key = (B, bool(conf))
        if key not in self._smooth_bufs:
            lab = torch.zeros((B, self.H, self.W), dtype=torch.uint8, device=self.device)
            self._smooth_bufs[key] = (lab, torch.zeros_like(lab) if conf else None)
        return self._smooth_bufs[key]

    def stable_buffers(self, B: int, crop_w: int, crop_h: int):
        """(layout table, the streams' carried state) of the label stabilisation; the state
        belongs to the crop alone, like the track state."""
        if B not in self._stable_tables:
            self._stable_tables[B] = hip_ops.label_stable_tables(self.track_counts(B), self.device)
        skey = (crop_w, crop_h)
        if skey not in self._stable_state:
            self._stable_state[skey] = torch.zeros(
                hip_ops.label_stable_state_bytes(self.stable_streams, crop_h, crop_w),
                dtype=torch.uint8, device=self.device)
        return self._stable_tables[B], self._stable_state[skey]

    def track_buffers(self, B: int, crop_w: int, crop_h: int):
        """(scratch, layout tables, [B, 4 + (6 | 7 + 2) region_cap] int32 rows with tracks, the
        streams' carried state) of the tracking kernels; the state belongs to the crop alone."""
        key = (B, crop_w, crop_h)
        if key not in self._track_bufs:
            tws = torch.zeros(hip_ops.region_tracks_workspace_bytes(B, crop_h, crop_w, self.region_cap),
                              dtype=torch.uint8, device=self.device)
            tables = hip_ops.region_track_tables(self.track_counts(B), self.device)
            wide = torch.zeros((B, 4 + self.out_words * self.region_cap), dtype=torch.int32,
                               device=self.device)
            self._track_bufs[key] = (tws, tables, wide)
        skey = (crop_w, crop_h)
        if skey not in self._track_state:
            self._track_state[skey] = torch.zeros(
                hip_ops.region_tracks_state_bytes(self.track_streams, crop_h, crop_w),
                dtype=torch.uint8, device=self.device)
        return self._track_bufs[key] + (self._track_state[skey],)

    def presence_buffers(self, B: int, crop_w: int, crop_h: int):
        """(workspace, [B, 4 + U region_cap] int32 presence words, the streams' carried dwell
        state or None without tracking) of the zone-presence kernels: static and shared like
        ``zone_buffers``; the state belongs to the crop alone. Every run writes every word."""
        key = (B, crop_w, crop_h)
        tr = bool(self.track_streams)
        if key not in self._presence_bufs:
            from . import presence as PR
            PR.check_geometry(crop_w, crop_h, self.presence_rows - 1, self.region_cap)
            ws = torch.zeros(hip_ops.zone_presence_workspace_bytes(B, crop_h, crop_w, tr),
                             dtype=torch.uint8, device=self.device)
            words = torch.zeros((B, PR.frame_words(self.region_cap, self.presence_rows, tr)),
                                dtype=torch.int32, device=self.device)
            self._presence_bufs[key] = (ws, words)
        skey = (crop_w, crop_h)
        if tr and skey not in self._presence_state:
            self._presence_state[skey] = torch.zeros(
                hip_ops.zone_presence_state_bytes(self.track_streams, self.region_cap, self.presence_rows),
                dtype=torch.uint8, device=self.device)
        return self._presence_bufs[key] + (self._presence_state.get(skey),)

    def event_buffers(self, B: int, crop_w: int, crop_h: int):
        """([B, 4 + 4 event_cap] int32 event words, the streams' carried presence rows) of the
        zone-event kernels: static and shared like ``presence_buffers``; the state belongs to the
        crop alone. Every run writes every word."""
        key = (B, crop_w, crop_h)
        if key not in self._event_bufs:
            from . import events as EV
            EV.check_geometry(self.event_cap)
            self._event_bufs[key] = torch.zeros((B, EV.frame_words(self.event_cap)), dtype=torch.int32,
                                                device=self.device)
        skey = (crop_w, crop_h)
        if skey not in self._event_state:
            self._event_state[skey] = torch.zeros(
                hip_ops.zone_events_state_bytes(self.track_streams, self.region_cap, self.presence_rows),
                dtype=torch.uint8, device=self.device)
        return self._event_bufs[key], self._event_state[skey]

    def reset_tracks(self) -> None:
        """Forget every stream's carried state (ids start again at 1, dwells at 0, the next
        frame's labels pass the stabilisation unchanged), once the device is idle."""
        if not self._track_state and not self._stable_state:
            return
        torch.cuda.synchronize(self.device)
        for st in (list(self._track_state.values()) + list(self._presence_state.values())
                   + list(self._event_state.values()) + list(self._stable_state.values())):
            st.zero_()
        torch.cuda.synchronize(self.device)

    def run(self, labels: torch.Tensor, crop_w: int, crop_h: int, min_area: float,
            out: torch.Tensor = None, mask_out: torch.Tensor = None,
            region_out: torch.Tensor = None, conf: torch.Tensor = None,
            zone_out: torch.Tensor = None, presence_out: torch.Tensor = None,
            event_out: torch.Tensor = None) -> torch.Tensor:
        """Packed records of ``labels`` into the static buffer for this B, or into ``out``
        ([B, 1 + 5K] fp32, e.g. a row slice of a bigger batch's buffer). The workspace is
        shared per B: runs that share it must be ordered on one stream. With ``mask_cap``
        the label maps are run-length encoded right after, on the same stream (so inside the
        same captured graph), into ``mask_buffers(B)`` or ``mask_out`` ([B, 4 + mask_cap]
        int32 rows); ``last_mask`` is the buffer written. With ``region_cap`` the class regions
        follow on the same stream, into ``region_buffers(B)`` or ``region_out`` ([B, 4 + 6
        region_cap] int32 rows); ``last_regions`` is the buffer written. With ``region_conf``,
        ``conf`` is the [B, H, W] uint8 confidence plane of ``labels`` and the rows are [B, 4 + 7
        region_cap]. With ``track_streams`` the rows are two words wider (track_id, age) and
        the frames of ``labels`` are the next ones of their streams, laid out by ``track_counts``.
        With ``zone_rows`` the zone occupancy comes last on the same stream, into
        ``zone_buffers(B)`` or ``zone_out`` ([B, 4 + R C] int32 rows, [B, 4 + 2 R C] with
        ``zone_conf``, which reads ``conf`` too); ``last_zones`` is the buffer written. With
        ``presence_rows`` the zone presence of the regions follows, into ``presence_buffers(B)`` or
        ``presence_out`` ([B, 4 + U region_cap] int32 rows); ``last_presence`` is the buffer
        written. With ``event_cap`` the zone events of the frames end the chain, into
        ``event_buffers(B)`` or ``event_out`` ([B, 4 + 4 event_cap] int32 rows); ``last_events`` is
        the buffer written. With ``stable_frames`` the label stabilisation comes first, on the same stream
        (the graph stays a chain): ``labels`` -- and ``conf``, when passed -- are overwritten in
        place with the stabilised planes, which everything above then reads; the frames are the
        next ones of their streams, laid out by ``track_counts``. With ``smooth_radius`` the label
        smoothing comes before that, out of place into ``smooth_buffers(B)``; the stabilisation
        then reads those planes, and without it they are copied back on the same stream: when
        ``run`` returns, ``labels`` and ``conf`` hold the smoothed (and stabilised) maps."""
        B = labels.shape[0]
        if labels.shape[1:] != (self.H, self.W):
            raise ValueError(f"labels {tuple(labels.shape)} != (B, {self.H}, {self.W})")
        if self.stable_frames and self.stable_gate and conf is None:
            raise ValueError("DevicePostprocess.run: stable_gate needs the conf plane")
        raw, raw_conf = labels, conf  # what the stabilisation reads
        if self.smooth_radius:
            raw, raw_conf = self.smooth_buffers(B, conf is not None)
            hip_ops.label_smooth(labels, raw, conf, raw_conf, B=B, H=self.H, W=self.W, crop_h=crop_h,
                                 crop_w=crop_w, R=self.smooth_radius)
            if not self.stable_frames:  # device to device, same stream: the graph stays a chain
                labels.copy_(raw)
                if conf is not None:
                    conf.copy_(raw_conf)
        if self.stable_frames:
            tables, state = self.stable_buffers(B, crop_w, crop_h)
            hip_ops.label_stable(raw, labels, raw_conf, conf, state, tables,
                                 counts=self.track_counts(B), B=B, H=self.H, W=self.W,
                                 crop_h=crop_h, crop_w=crop_w, N=self.stable_frames,
                                 g=self.stable_gate)
        ws, rec = self._buffers(B)
        if out is not None:
            if (out.shape != rec.shape or out.dtype != rec.dtype or not out.is_contiguous()
                    or out.device != rec.device):
                raise ValueError("DevicePostprocess.run: out must be a contiguous [B, 1 + 5K] fp32 buffer")
            rec = out
        hip_ops.postprocess(labels, self.palette, ws, rec, B=B, H=self.H, W=self.W, crop_h=crop_h,
                            crop_w=crop_w, min_area=min_area, K=self.K, bins=self.bins, thr=self.thr,
                            accum=self.accum_for(B))
        if self.mask_cap:
            mws, words = self.mask_buffers(B, crop_w, crop_h)
            if mask_out is not None:
                words = mask_out
            hip_ops.mask_rle(labels, words, mws, B=B, H=self.H, W=self.W, crop_h=crop_h,
                             crop_w=crop_w, cap=self.mask_cap)
            self.last_mask = words
        if self.region_cap:
            rws, words = self.region_buffers(B, crop_w, crop_h)
            if region_out is not None and not self.track_streams:
                words = region_out
            if self.region_conf and conf is None:
                raise ValueError("DevicePostprocess.run: region_conf needs the conf plane")
            hip_ops.class_regions(labels, words, rws, B=B, H=self.H, W=self.W, crop_h=crop_h,
                                  crop_w=crop_w, classes=self.region_classes,
                                  min_pixels=self.region_min_pixels, K=self.region_cap,
                                  conf=conf if self.region_conf else None)
            if self.track_streams:  # same stream, same graph: the rows with track_id and age
                tws, tables, wide, state = self.track_buffers(B, crop_w, crop_h)
                if region_out is not None:
                    wide = region_out
                hip_ops.region_tracks(words, wide, rws, tws, state, tables,
                                      counts=self.track_counts(B), crop_h=crop_h, crop_w=crop_w,
                                      K=self.region_cap, q=self.track_q, conf=self.region_conf)
                words = wide
            self.last_regions = words
        if self.zone_rows:
            zws, words = self.zone_buffers(B, crop_w, crop_h)
            if zone_out is not None:
                words = zone_out
            if self.zone_conf and conf is None:
                raise ValueError("DevicePostprocess.run: zone_conf needs the conf plane")
            plane = None
            if self.zone_rows > 1:
                plane = self._zone_plane.get((crop_w, crop_h))
                if plane is None:
                    raise ValueError(f"DevicePostprocess.run: no zone plane set for the {crop_w} x "
                                     f"{crop_h} crop (set_zone_plane)")
            hip_ops.zone_stats(labels, words, zws, B=B, H=self.H, W=self.W, crop_h=crop_h,
                               crop_w=crop_w, R=self.zone_rows, C=self.zone_classes, plane=plane,
                               conf=conf if self.zone_conf else None)
            self.last_zones = words
        if self.presence_rows:
            pws, words, pstate = self.presence_buffers(B, crop_w, crop_h)
            if presence_out is not None:
                words = presence_out
            kw = {}
            if self.track_streams:
                tws, tables, _, _ = self.track_buffers(B, crop_w, crop_h)
                kw = dict(tws=tws, state=pstate, tables=tables, counts=self.track_counts(B),
                          q=self.presence_q)
            hip_ops.zone_presence(self.last_regions, words, pws, rws, B=B, crop_h=crop_h, crop_w=crop_w,
                                  K=self.region_cap, R=self.presence_rows, plane=plane,
                                  conf=self.region_conf, **kw)
            self.last_presence = words
        if self.event_cap:
            ewords, estate = self.event_buffers(B, crop_w, crop_h)
            if event_out is not None:
                ewords = event_out
            hip_ops.zone_events(self.last_presence, ewords, estate, tables,
                                counts=self.track_counts(B), K=self.region_cap,
                                R=self.presence_rows, E=self.event_cap)
            self.last_events = ewords
        return rec

    def fetch(self, rec: torch.Tensor, frame_ids: Sequence[int], ts: Sequence[float],
              streams: Sequence[int], W: int, H: int) -> np.ndarray:
        from ..parallel.dp import unpack_records
        B = rec.shape[0]
        h = self._host.get(B)
        if h is None:
            h = self._host[B] = torch.empty(rec.shape, dtype=torch.float32, pin_memory=True)
        h.copy_(rec, non_blocking=True)
        torch.cuda.current_stream(self.device).synchronize()
        return unpack_records(h.numpy(), self.K, frame_ids, ts, streams)

    def fetch_masks(self, words: torch.Tensor) -> np.ndarray:
        """Synchronous D2H of the run words (or the region words) of ``run`` -> uint32 of the
        same shape (a copy)."""
        key = tuple(words.shape)
        h = self._mask_host.get(key)
        if h is None:
            h = self._mask_host[key] = torch.empty(words.shape, dtype=torch.int32, pin_memory=True)
        h.copy_(words, non_blocking=True)
        torch.cuda.current_stream(self.device).synchronize()
        return h.numpy().view(np.uint32).copy()

    fetch_regions = fetch_masks  # the same: a uint32 row per frame with a 4-word header
    fetch_zones = fetch_masks
    fetch_presence = fetch_masks
    fetch_events = fetch_masks
