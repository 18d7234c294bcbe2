"""gRPC servicers, registration helpers and client stubs.

v1 ``sem_seg_server.SemanticSegmentation`` mirrors the reference servicer
(``sem_seg_server.py:216-234``) and its generated registration/stub code
(``sem_seg_server_pb2_grpc.py:8-63``): two unary-unary methods with ``Empty``
requests, ``GetSegmentedObjects`` pops exactly ``num_detections`` records
newest-first and pads with default ``SegmentedObject()`` messages, and
``GetCameraResolution`` returns the resolution probed once at startup. The RPC
never waits on inference.

v2 ``sem_seg_server.v2.SemanticSegmentationV2`` is new: per-stream reads with
frame ids/timestamps, stream listing, stats and health.
"""
from __future__ import annotations

import json
import time
from concurrent import futures
from typing import Callable, Dict, Optional, Tuple

import grpc
import numpy as np

from . import proto as P
from ..labels import label_name
from ..runtime.results import ResultHub


def _obj(rec, labels) -> "P.SegmentedObject":
    return P.SegmentedObject(
        label=label_name(labels, int(rec["label"])),
        score=float(rec["score"]),
        area=float(rec["area"]),
        centroid=P.Centroid(cx=float(rec["cx"]), cy=float(rec["cy"])),
    )


class SemanticSegmentationServicer:
    """v1 service (reference-compatible)."""

    def __init__(self, hub: ResultHub, labels: Dict[int, str], num_detections: int = 3,
                 camera_res: Tuple[int, int] = (0, 0), stream: int = 0, metrics=None):
        self.hub = hub
        self.labels = labels
        self.num_detections = int(num_detections)
        self.camera_res = camera_res
        self.stream = stream
        self.metrics = metrics

    def GetCameraResolution(self, request, context):
        return P.CameraResolution(width=int(self.camera_res[0]), height=int(self.camera_res[1]))

    def GetSegmentedObjects(self, request, context):
        t0 = time.perf_counter()
        recs = self.hub.buffer(self.stream).pop(self.num_detections)
        data = [_obj(r, self.labels) for r in recs]
        data.extend(P.SegmentedObject() for _ in range(self.num_detections - len(data)))
        out = P.SegmentedObjectData(data=data)
        if self.metrics is not None:
            self.metrics.observe("rpc_get_segmented_objects_ms", (time.perf_counter() - t0) * 1e3)
        return out


MAX_V2_OBJECTS = 4096  # per-request cap of GetStreamSegmentedObjects (padding included)
MAX_V2_EVENTS = 1024   # GetZoneEvents' max_events when the request leaves it 0


class SemanticSegmentationV2Servicer:
    """v2 extension service. Client input is bounded: ``max_objects`` is clamped to
    [0, min(buffer capacity, MAX_V2_OBJECTS)] (a huge padded request would otherwise
    build billions of messages on the node's only RPC host) and an unknown
    ``stream_id`` is NOT_FOUND instead of creating a buffer."""

    def __init__(self, hub: ResultHub, labels: Dict[int, str], num_detections: int = 3,
                 streams: Optional[list] = None, metrics=None,
                 health_fn: Optional[Callable[[], Tuple[bool, int, int, str]]] = None, *,
                 serve_masks: bool = False, model_size: Tuple[int, int] = (0, 0),
                 serve_regions: bool = False, zone_names: Optional[list] = None,
                 presence_q: int = 0, serve_events: bool = False):
        self.hub = hub
        # --serve_events: GetZoneEvents is enabled (the rows are those of zone_names)
        self.serve_events = bool(serve_events)
        # --serve_presence: q of --presence_min_share (0: GetZonePresence is off); the rows are
        # those of zone_names, and every stored item says whether it carries tracks
        self.presence_q = int(presence_q)
        # --serve_zones: the names of the zone rows, "frame" first (None: GetZoneOccupancy is off)
        self.zone_names = list(zone_names) if zone_names else None
        self.serve_regions = bool(serve_regions)  # --serve_regions: GetClassRegions is enabled
        self.serve_masks = bool(serve_masks)  # --serve_masks: GetSegmentationMask is enabled
        self.model_size = model_size          # (width, height) of the label maps
        self.labels = labels
        self.num_detections = int(num_detections)
        self.streams = streams or []
        self.metrics = metrics
        self.health_fn = health_fn

    def GetStreamSegmentedObjects(self, request, context):
        buf = self.hub.get(int(request.stream_id))
        if buf is None:
            context.set_code(grpc.StatusCode.NOT_FOUND)
            context.set_details(f"unknown stream_id {request.stream_id}")
            return P.StreamSegmentedObjects()
        cap = min(MAX_V2_OBJECTS, buf.maxlen or MAX_V2_OBJECTS)
        n = max(0, min(int(request.max_objects or self.num_detections), cap))
        recs = buf.pop(n)
        data = [P.TaggedObject(object=_obj(r, self.labels), frame_id=int(r["frame"]),
                               timestamp=float(r["ts"]), stream_id=int(r["stream"]))
                for r in recs]
        if request.pad:
            data.extend(P.TaggedObject(stream_id=request.stream_id) for _ in range(n - len(data)))
        return P.StreamSegmentedObjects(data=data)

    def GetSegmentationMask(self, request, context):
        """The stream's latest label mask. The producer stores run starts; the lengths of
        the wire format are taken here, for the one mask an RPC asks for."""
        from ..postprocess import mask_rle as MR
        stream = int(request.stream_id)
        if not self.serve_masks:
            context.set_code(grpc.StatusCode.FAILED_PRECONDITION)
            context.set_details("label masks are not enabled (start the server with --serve_masks)")
            return P.SegmentationMask()
        if self.hub.get(stream) is None:
            context.set_code(grpc.StatusCode.NOT_FOUND)
            context.set_details(f"unknown stream_id {request.stream_id}")
            return P.SegmentationMask()
        m = self.hub.mask(stream)
        if m is None:
            context.set_code(grpc.StatusCode.UNAVAILABLE)
            context.set_details(f"no frame of stream {stream} collected yet")
            return P.SegmentationMask()
        labs, lens, truncated, total = MR.to_wire(m.words)
        return P.SegmentationMask(
            stream_id=stream, frame_id=m.frame_id, timestamp=m.ts, width=int(m.words[2]),
            height=int(m.words[3]), model_width=int(self.model_size[0]),
            model_height=int(self.model_size[1]), run_labels=labs, run_lengths=lens.tolist(),
            truncated=truncated, total_runs=total)

    def GetClassRegions(self, request, context):
        """The connected same-class regions of the stream's latest frame, largest first. The
        producer stores integer words (postprocess/regions.py); the floats of the wire format
        are computed here, for the one stream an RPC asks for."""
        from ..postprocess import regions as RG
        stream = int(request.stream_id)
        if not self.serve_regions:
            context.set_code(grpc.StatusCode.FAILED_PRECONDITION)
            context.set_details("class regions are not enabled (start the server with --serve_regions)")
            return P.ClassRegions()
        if self.hub.get(stream) is None:
            context.set_code(grpc.StatusCode.NOT_FOUND)
            context.set_details(f"unknown stream_id {request.stream_id}")
            return P.ClassRegions()
        r = self.hub.regions(stream)
        if r is None:
            context.set_code(grpc.StatusCode.UNAVAILABLE)
            context.set_details(f"no frame of stream {stream} collected yet")
            return P.ClassRegions()
        has_conf = bool(getattr(r, "conf", False))
        has_tracks = bool(getattr(r, "tracks", False))
        tab = RG.decode(r.words, conf=has_conf, tracks=has_tracks)
        total = int(r.words[0])
        if request.max_regions > 0:
            tab = tab[:int(request.max_regions)]
        mw, mh = float(self.model_size[0]), float(self.model_size[1])
        out = []
        for t in tab:
            px = int(t["pixels"])
            out.append(P.ClassRegion(
                label=label_name(self.labels, int(t["label"])), class_id=int(t["label"]), pixels=px,
                area=px / (mw * mh), cx=(int(t["sum_x"]) / px + 0.5) / mw,
                cy=(int(t["sum_y"]) / px + 0.5) / mh, x_min=int(t["x_min"]) / mw,
                y_min=int(t["y_min"]) / mh, x_max=(int(t["x_max"]) + 1) / mw,
                y_max=(int(t["y_max"]) + 1) / mh,
                confidence=int(t["sum_conf"]) / (255 * px) if has_conf else 0.0,
                track_id=int(t["track_id"]), age=int(t["age"])))
        return P.ClassRegions(
            stream_id=stream, frame_id=r.frame_id, timestamp=r.ts, width=int(r.words[2]),
            height=int(r.words[3]), model_width=int(self.model_size[0]),
            model_height=int(self.model_size[1]), regions=out, total_regions=total,
            truncated=len(out) < total, has_confidence=has_conf, has_tracks=has_tracks)

    def GetZoneOccupancy(self, request, context):
        """The pixels of every class inside every zone of the stream's latest frame. The
        producer stores integer counts (postprocess/zones.py); the floats of the wire format
        are computed here, for the one stream an RPC asks for."""
        from ..postprocess import zones as ZN
        stream = int(request.stream_id)
        if self.zone_names is None:
            context.set_code(grpc.StatusCode.FAILED_PRECONDITION)
            context.set_details("zone occupancy is not enabled (start the server with --serve_zones)")
            return P.ZoneOccupancy()
        if self.hub.get(stream) is None:
            context.set_code(grpc.StatusCode.NOT_FOUND)
            context.set_details(f"unknown stream_id {request.stream_id}")
            return P.ZoneOccupancy()
        z = self.hub.zones(stream)
        if z is None:
            context.set_code(grpc.StatusCode.UNAVAILABLE)
            context.set_details(f"no frame of stream {stream} collected yet")
            return P.ZoneOccupancy()
        has_conf = bool(z.conf)
        st = ZN.decode(z.words, conf=has_conf)
        out = []
        for r in range(st.rows):
            px = st.pixels[r].astype(np.int64)
            total = int(px.sum())
            ids = [int(c) for c in np.lexsort((np.arange(len(px)), -px)) if px[c] > 0]
            classes = [P.ZoneClass(
                class_id=c, label=label_name(self.labels, c), pixels=int(px[c]),
                share=int(px[c]) / total,
                confidence=int(st.sum_conf[r, c]) / (255 * int(px[c])) if has_conf else 0.0) for c in ids]
            out.append(P.Zone(index=r, name=self.zone_names[r] if r < len(self.zone_names) else str(r),
                              pixels=total, area=total / st.n if st.n else 0.0, classes=classes))
        return P.ZoneOccupancy(
            stream_id=stream, frame_id=z.frame_id, timestamp=z.ts, width=st.crop_w, height=st.crop_h,
            model_width=int(self.model_size[0]), model_height=int(self.model_size[1]), zones=out,
            has_confidence=has_conf)

    def GetZonePresence(self, request, context):
        """The pixels of every class region inside every zone of the stream's latest frame. The
        producer stores integers (postprocess/presence.py); share and inside are computed here
        from them, for the one stream an RPC asks for."""
        from ..postprocess import presence as PR
        stream = int(request.stream_id)
        if not self.presence_q or self.zone_names is None:
            context.set_code(grpc.StatusCode.FAILED_PRECONDITION)
            context.set_details("zone presence is not enabled (start the server with --serve_presence)")
            return P.ZonePresence()
        if self.hub.get(stream) is None:
            context.set_code(grpc.StatusCode.NOT_FOUND)
            context.set_details(f"unknown stream_id {request.stream_id}")
            return P.ZonePresence()
        z = self.hub.presence(stream)
        if z is None:
            context.set_code(grpc.StatusCode.UNAVAILABLE)
            context.set_details(f"no frame of stream {stream} collected yet")
            return P.ZonePresence()
        tr = bool(z.tracks)
        pr = PR.decode(z.words, len(self.zone_names), tracks=tr)
        ins = PR.inside(pr.P, self.presence_q)
        out = []
        for a in range(pr.n):
            px = int(pr.P[a, 0])
            hits = [P.ZoneHit(index=r, name=self.zone_names[r], pixels=int(pr.P[a, r]),
                              share=int(pr.P[a, r]) / px if px else 0.0, inside=bool(ins[a, r]),
                              dwell=int(pr.D[a, r]) if tr else 0)
                    for r in range(1, pr.P.shape[1]) if pr.P[a, r] > 0]
            out.append(P.RegionPresence(index=a, label=label_name(self.labels, int(pr.label[a])),
                                        class_id=int(pr.label[a]), root=int(pr.root[a]), pixels=px,
                                        track_id=int(pr.track_id[a]), age=int(pr.D[a, 0]) if tr else 0,
                                        zones=hits))
        return P.ZonePresence(
            stream_id=stream, frame_id=z.frame_id, timestamp=z.ts, width=pr.crop_w, height=pr.crop_h,
            model_width=int(self.model_size[0]), model_height=int(self.model_size[1]), regions=out,
            has_tracks=tr, min_share=self.presence_q / PR.Q_ONE)

    def GetZoneEvents(self, request, context):
        """A stretch of the stream's event log after the cursor ``after_seq``: a log, so an empty
        answer with ``next_seq == after_seq`` is ordinary. The ``zones`` filter applies after the
        cursor: the sequence numbers of an answer may have gaps."""
        from ..postprocess import events as EV
        from ..postprocess import presence as PR
        stream = int(request.stream_id)
        if not self.serve_events or self.zone_names is None:
            context.set_code(grpc.StatusCode.FAILED_PRECONDITION)
            context.set_details("zone events are not enabled (start the server with --serve_events)")
            return P.ZoneEvents()
        if self.hub.get(stream) is None:
            context.set_code(grpc.StatusCode.NOT_FOUND)
            context.set_details(f"unknown stream_id {request.stream_id}")
            return P.ZoneEvents()
        limit = max(1, min(int(request.max_events) or MAX_V2_EVENTS, self.hub.event_log))
        rows, next_seq, lost = self.hub.events_after(stream, int(request.after_seq), limit)
        if len(request.zones):
            ev = EV.decode(np.stack([rows["w0"], rows["w1"], rows["w2"], rows["w3"]], 1))
            rows = rows[np.isin(ev["zone"], np.array(list(request.zones), np.int64))]
        ev = EV.decode(np.stack([rows["w0"], rows["w1"], rows["w2"], rows["w3"]], 1))
        nz = len(self.zone_names)
        out = []
        for r, e in zip(rows, ev):
            z, enter = int(e["zone"]), int(e["kind"]) == EV.ENTER
            out.append(P.ZoneEvent(
                seq=int(r["seq"]), epoch=int(r["epoch"]), kind=int(e["kind"]), frame_id=int(r["frame_id"]),
                timestamp=float(r["ts"]), zone=z, zone_name=self.zone_names[z] if z < nz else "",
                track_id=int(e["track_id"]), class_id=int(e["label"]),
                label=label_name(self.labels, int(e["label"])), root=int(e["root"]),
                track_edge=bool(e["edge"]), pixels=int(e["value"]) if enter else 0,
                dwell=0 if enter else int(e["value"])))
        return P.ZoneEvents(stream_id=stream, events=out, next_seq=next_seq, lost=lost,
                            truncated=self.hub.events_truncated(stream),
                            min_share=self.presence_q / PR.Q_ONE)

    def ListStreams(self, request, context):
        return P.StreamList(streams=[P.StreamInfo(**s) for s in self.streams])

    def GetStats(self, request, context):
        snap = self.metrics.snapshot() if self.metrics is not None else {}
        fl = snap.get("frame_ms", {})
        return P.Stats(
            frames=int(snap.get("frames", 0)), fps=float(snap.get("fps", 0.0)),
            p50_frame_ms=float(fl.get("p50", 0.0)), p99_frame_ms=float(fl.get("p99", 0.0)),
            objects=int(snap.get("objects", 0)), buffer_depth=self.hub.depth,
            buffer_drops=self.hub.drops, json=json.dumps(snap, default=float))

    def Health(self, request, context):
        if self.health_fn is None:
            return P.HealthStatus(serving=True, ranks_alive=1, world_size=1, detail="ok")
        ok, alive, world, detail = self.health_fn()
        return P.HealthStatus(serving=ok, ranks_alive=alive, world_size=world, detail=detail)


def _handlers(servicer, methods: Dict[str, tuple]) -> Dict[str, grpc.RpcMethodHandler]:
    return {
        name: grpc.unary_unary_rpc_method_handler(
            getattr(servicer, name),
            request_deserializer=req.FromString,
            response_serializer=resp.SerializeToString)
        for name, (req, resp) in methods.items()
    }


def add_v1_servicer(servicer, server) -> None:
    server.add_generic_rpc_handlers(
        (grpc.method_handlers_generic_handler(P.V1_SERVICE, _handlers(servicer, P.V1_METHODS)),))


def add_v2_servicer(servicer, server) -> None:
    server.add_generic_rpc_handlers(
        (grpc.method_handlers_generic_handler(P.V2_SERVICE, _handlers(servicer, P.V2_METHODS)),))


class HealthServicer:
    """grpc.health.v1.Health. ``status_fn(service) -> bool | None`` (None = unknown
    service); "" and the two segmentation services are known. Watch streams the
    status whenever it changes (polled every ``watch_period`` s) until cancelled."""

    KNOWN = ("", P.V1_SERVICE, P.V2_SERVICE)

    def __init__(self, status_fn: Optional[Callable[[str], Optional[bool]]] = None,
                 watch_period: float = 0.5):
        self.status_fn = status_fn or (lambda service: True)
        self.watch_period = watch_period

    def _status(self, service: str) -> int:
        R = P.HealthCheckResponse
        if service not in self.KNOWN:
            return R.SERVICE_UNKNOWN
        ok = self.status_fn(service)
        return R.UNKNOWN if ok is None else (R.SERVING if ok else R.NOT_SERVING)

    def Check(self, request, context):
        st = self._status(request.service)
        if st == P.HealthCheckResponse.SERVICE_UNKNOWN:
            context.set_code(grpc.StatusCode.NOT_FOUND)
            context.set_details(f"unknown service {request.service!r}")
        return P.HealthCheckResponse(status=st)

    def Watch(self, request, context):
        last = None
        while context.is_active():
            st = self._status(request.service)
            if st != last:
                yield P.HealthCheckResponse(status=st)
                last = st
            time.sleep(self.watch_period)


def add_health_servicer(servicer: HealthServicer, server) -> None:
    handlers = {
        "Check": grpc.unary_unary_rpc_method_handler(
            servicer.Check, request_deserializer=P.HealthCheckRequest.FromString,
            response_serializer=P.HealthCheckResponse.SerializeToString),
        "Watch": grpc.unary_stream_rpc_method_handler(
            servicer.Watch, request_deserializer=P.HealthCheckRequest.FromString,
            response_serializer=P.HealthCheckResponse.SerializeToString),
    }
    server.add_generic_rpc_handlers((grpc.method_handlers_generic_handler(P.HEALTH_SERVICE, handlers),))


class HealthStub:
    def __init__(self, channel):
        self.Check = channel.unary_unary(
            f"/{P.HEALTH_SERVICE}/Check", request_serializer=P.HealthCheckRequest.SerializeToString,
            response_deserializer=P.HealthCheckResponse.FromString)
        self.Watch = channel.unary_stream(
            f"/{P.HEALTH_SERVICE}/Watch", request_serializer=P.HealthCheckRequest.SerializeToString,
            response_deserializer=P.HealthCheckResponse.FromString)


class _Stub:
    def __init__(self, channel, service: str, methods: Dict[str, tuple]):
        for name, (req, resp) in methods.items():
            setattr(self, name, channel.unary_unary(
                f"/{service}/{name}",
                request_serializer=req.SerializeToString,
                response_deserializer=resp.FromString))


class SemanticSegmentationStub(_Stub):
    def __init__(self, channel):
        super().__init__(channel, P.V1_SERVICE, P.V1_METHODS)


class SemanticSegmentationV2Stub(_Stub):
    def __init__(self, channel):
        super().__init__(channel, P.V2_SERVICE, P.V2_METHODS)


def make_server(max_workers: int = 10, port: int = 50051, host: str = "[::]"):
    """grpc.server on its own thread pool (the reference shares one 10-thread pool
    between the producer and the RPC handlers, ``sem_seg_server.py:272-278``)."""
    server = grpc.server(futures.ThreadPoolExecutor(max_workers=max_workers),
                         options=[("grpc.so_reuseport", 0)])
    bound = server.add_insecure_port(f"{host}:{port}")
    return server, bound
