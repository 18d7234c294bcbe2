"""Protobuf message classes for the segmentation API, built without protoc.

The reference ships protoc-generated modules (``sem_seg_server_pb2.py``,
``sem_seg_server_pb2_grpc.py``) that only import under protobuf 3.x; protobuf in
this image is 7.x and there is no ``grpc_tools``. We therefore describe the two
files (``sem_seg_server.proto`` and the v2 extension) with ``descriptor_pb2``,
register them in a private ``DescriptorPool`` and materialise message classes with
``message_factory.GetMessageClass``. The resulting v1 wire format is identical to
the reference's (field numbers/types of ``sem_seg_server.proto:14-50``), which
``tests/test_api.py`` checks against hand-encoded bytes.
"""
from __future__ import annotations

from google.protobuf import descriptor_pb2, descriptor_pool, message_factory

F = descriptor_pb2.FieldDescriptorProto

PACKAGE = "sem_seg_server"
V1_SERVICE = "sem_seg_server.SemanticSegmentation"
V2_PACKAGE = "sem_seg_server.v2"
V2_SERVICE = "sem_seg_server.v2.SemanticSegmentationV2"


def _field(msg, name, number, ftype, label=F.LABEL_OPTIONAL, type_name=None):
    f = msg.field.add()
    f.name = name
    f.number = number
    f.type = ftype
    f.label = label
    if type_name:
        f.type_name = type_name
    # proto3 JSON name convention
    parts = name.split("_")
    f.json_name = parts[0] + "".join(p.title() for p in parts[1:])
    return f


def _method(svc, name, inp, out):
    m = svc.method.add()
    m.name = name
    m.input_type = inp
    m.output_type = out
    return m


def v1_file_descriptor() -> descriptor_pb2.FileDescriptorProto:
    fd = descriptor_pb2.FileDescriptorProto()
    fd.name = "sem_seg_server.proto"
    fd.package = PACKAGE
    fd.syntax = "proto3"

    so = fd.message_type.add()
    so.name = "SegmentedObject"
    cen = so.nested_type.add()
    cen.name = "Centroid"
    _field(cen, "cx", 1, F.TYPE_FLOAT)
    _field(cen, "cy", 2, F.TYPE_FLOAT)
    _field(so, "label", 1, F.TYPE_STRING)
    _field(so, "score", 2, F.TYPE_FLOAT)
    _field(so, "area", 3, F.TYPE_FLOAT)
    _field(so, "centroid", 4, F.TYPE_MESSAGE,
           type_name=".sem_seg_server.SegmentedObject.Centroid")

    sod = fd.message_type.add()
    sod.name = "SegmentedObjectData"
    _field(sod, "data", 1, F.TYPE_MESSAGE, F.LABEL_REPEATED, ".sem_seg_server.SegmentedObject")

    cr = fd.message_type.add()
    cr.name = "CameraResolution"
    _field(cr, "width", 1, F.TYPE_INT32)
    _field(cr, "height", 2, F.TYPE_INT32)

    em = fd.message_type.add()
    em.name = "Empty"

    svc = fd.service.add()
    svc.name = "SemanticSegmentation"
    _method(svc, "GetSegmentedObjects", ".sem_seg_server.Empty", ".sem_seg_server.SegmentedObjectData")
    _method(svc, "GetCameraResolution", ".sem_seg_server.Empty", ".sem_seg_server.CameraResolution")
    return fd


def v2_file_descriptor() -> descriptor_pb2.FileDescriptorProto:
    fd = descriptor_pb2.FileDescriptorProto()
    fd.name = "sem_seg_server_v2.proto"
    fd.package = V2_PACKAGE
    fd.syntax = "proto3"
    fd.dependency.append("sem_seg_server.proto")
    P = "." + V2_PACKAGE + "."

    m = fd.message_type.add(); m.name = "StreamRequest"
    _field(m, "stream_id", 1, F.TYPE_INT32)
    _field(m, "max_objects", 2, F.TYPE_INT32)
    _field(m, "pad", 3, F.TYPE_BOOL)

    m = fd.message_type.add(); m.name = "TaggedObject"
    _field(m, "object", 1, F.TYPE_MESSAGE, type_name=".sem_seg_server.SegmentedObject")
    _field(m, "frame_id", 2, F.TYPE_INT64)
    _field(m, "timestamp", 3, F.TYPE_DOUBLE)
    _field(m, "stream_id", 4, F.TYPE_INT32)

    m = fd.message_type.add(); m.name = "StreamSegmentedObjects"
    _field(m, "data", 1, F.TYPE_MESSAGE, F.LABEL_REPEATED, P + "TaggedObject")

    m = fd.message_type.add(); m.name = "StreamInfo"
    _field(m, "stream_id", 1, F.TYPE_INT32)
    _field(m, "width", 2, F.TYPE_INT32)
    _field(m, "height", 3, F.TYPE_INT32)
    _field(m, "rank", 4, F.TYPE_INT32)
    _field(m, "source", 5, F.TYPE_STRING)

    m = fd.message_type.add(); m.name = "StreamList"
    _field(m, "streams", 1, F.TYPE_MESSAGE, F.LABEL_REPEATED, P + "StreamInfo")

    m = fd.message_type.add(); m.name = "Stats"
    _field(m, "frames", 1, F.TYPE_INT64)
    _field(m, "fps", 2, F.TYPE_DOUBLE)
    _field(m, "p50_frame_ms", 3, F.TYPE_DOUBLE)
    _field(m, "p99_frame_ms", 4, F.TYPE_DOUBLE)
    _field(m, "objects", 5, F.TYPE_INT64)
    _field(m, "buffer_depth", 6, F.TYPE_INT64)
    _field(m, "buffer_drops", 7, F.TYPE_INT64)
    _field(m, "json", 8, F.TYPE_STRING)

    m = fd.message_type.add(); m.name = "HealthStatus"
    _field(m, "serving", 1, F.TYPE_BOOL)
    _field(m, "ranks_alive", 2, F.TYPE_INT32)
    _field(m, "world_size", 3, F.TYPE_INT32)
    _field(m, "detail", 4, F.TYPE_STRING)

    m = fd.message_type.add(); m.name = "MaskRequest"
    _field(m, "stream_id", 1, F.TYPE_INT32)

    # the stream's latest label mask, run-length encoded over the flat row-major crop
    # region (postprocess/mask_rle.py): run k covers run_lengths[k] pixels of class
    # run_labels[k]; the lengths sum to width * height unless truncated
    m = fd.message_type.add(); m.name = "SegmentationMask"
    _field(m, "stream_id", 1, F.TYPE_INT32)
    _field(m, "frame_id", 2, F.TYPE_INT64)
    _field(m, "timestamp", 3, F.TYPE_DOUBLE)
    _field(m, "width", 4, F.TYPE_INT32)    # crop region, model-resolution pixels
    _field(m, "height", 5, F.TYPE_INT32)
    _field(m, "model_width", 6, F.TYPE_INT32)
    _field(m, "model_height", 7, F.TYPE_INT32)
    _field(m, "run_labels", 8, F.TYPE_BYTES)  # one class id per run
    _field(m, "run_lengths", 9, F.TYPE_UINT32, F.LABEL_REPEATED)  # packed (proto3)
    _field(m, "truncated", 10, F.TYPE_BOOL)
    _field(m, "total_runs", 11, F.TYPE_UINT32)

    m = fd.message_type.add(); m.name = "RegionRequest"
    _field(m, "stream_id", 1, F.TYPE_INT32)
    _field(m, "max_regions", 2, F.TYPE_INT32)  # 0: all stored

    # one 8-connected set of pixels of one class (postprocess/regions.py); the floats are
    # fractions of the model input, like v1's area and centroid axes
    m = fd.message_type.add(); m.name = "ClassRegion"
    _field(m, "label", 1, F.TYPE_STRING)
    _field(m, "class_id", 2, F.TYPE_INT32)
    _field(m, "pixels", 3, F.TYPE_UINT32)
    _field(m, "area", 4, F.TYPE_FLOAT)    # pixels / (model_width * model_height)
    _field(m, "cx", 5, F.TYPE_FLOAT)      # (sum / pixels + 0.5) / model size
    _field(m, "cy", 6, F.TYPE_FLOAT)
    _field(m, "x_min", 7, F.TYPE_FLOAT)   # box edges / model size; the max edges are exclusive
    _field(m, "y_min", 8, F.TYPE_FLOAT)
    _field(m, "x_max", 9, F.TYPE_FLOAT)
    _field(m, "y_max", 10, F.TYPE_FLOAT)
    # mean winning-class softmax probability of the region's pixels (--serve_confidence; else 0)
    _field(m, "confidence", 11, F.TYPE_FLOAT)
    # identity of the region across the stream's frames and the frames it has lived
    # (--track_regions, postprocess/tracks.py; else 0)
    _field(m, "track_id", 12, F.TYPE_UINT32)
    _field(m, "age", 13, F.TYPE_UINT32)

    # the regions of the stream's latest frame, by (pixels descending, first pixel ascending)
    m = fd.message_type.add(); m.name = "ClassRegions"
    _field(m, "stream_id", 1, F.TYPE_INT32)
    _field(m, "frame_id", 2, F.TYPE_INT64)
    _field(m, "timestamp", 3, F.TYPE_DOUBLE)
    _field(m, "width", 4, F.TYPE_INT32)    # crop region, model-resolution pixels
    _field(m, "height", 5, F.TYPE_INT32)
    _field(m, "model_width", 6, F.TYPE_INT32)
    _field(m, "model_height", 7, F.TYPE_INT32)
    _field(m, "regions", 8, F.TYPE_MESSAGE, F.LABEL_REPEATED, ".sem_seg_server.v2.ClassRegion")
    _field(m, "total_regions", 9, F.TYPE_UINT32)  # regions that passed; more than stored: truncated
    _field(m, "truncated", 10, F.TYPE_BOOL)
    _field(m, "has_confidence", 11, F.TYPE_BOOL)  # the regions carry a confidence
    _field(m, "has_tracks", 12, F.TYPE_BOOL)      # the regions carry track_id and age

    m = fd.message_type.add(); m.name = "ZoneRequest"
    _field(m, "stream_id", 1, F.TYPE_INT32)

    # one class present in one zone (postprocess/zones.py); the floats are computed from the
    # stored integer counts
    m = fd.message_type.add(); m.name = "ZoneClass"
    _field(m, "class_id", 1, F.TYPE_INT32)
    _field(m, "label", 2, F.TYPE_STRING)
    _field(m, "pixels", 3, F.TYPE_UINT32)
    _field(m, "share", 4, F.TYPE_FLOAT)       # pixels / the zone's pixels
    _field(m, "confidence", 5, F.TYPE_FLOAT)  # sum_conf / (255 * pixels); 0 without has_confidence

    m = fd.message_type.add(); m.name = "Zone"
    _field(m, "index", 1, F.TYPE_INT32)       # 0: the implicit whole-frame zone "frame"
    _field(m, "name", 2, F.TYPE_STRING)
    _field(m, "pixels", 3, F.TYPE_UINT32)     # the sum over the classes: zone within the crop
    _field(m, "area", 4, F.TYPE_FLOAT)        # pixels / (width * height)
    # the classes with pixels > 0, by (pixels descending, class_id ascending)
    _field(m, "classes", 5, F.TYPE_MESSAGE, F.LABEL_REPEATED, P + "ZoneClass")

    # the class x zone pixel counts of the stream's latest frame
    m = fd.message_type.add(); m.name = "ZoneOccupancy"
    _field(m, "stream_id", 1, F.TYPE_INT32)
    _field(m, "frame_id", 2, F.TYPE_INT64)
    _field(m, "timestamp", 3, F.TYPE_DOUBLE)
    _field(m, "width", 4, F.TYPE_INT32)    # crop region, model-resolution pixels
    _field(m, "height", 5, F.TYPE_INT32)
    _field(m, "model_width", 6, F.TYPE_INT32)
    _field(m, "model_height", 7, F.TYPE_INT32)
    _field(m, "zones", 8, F.TYPE_MESSAGE, F.LABEL_REPEATED, P + "Zone")
    _field(m, "has_confidence", 9, F.TYPE_BOOL)  # the classes carry a confidence

    m = fd.message_type.add(); m.name = "PresenceRequest"
    _field(m, "stream_id", 1, F.TYPE_INT32)

    # one user zone a region has pixels in (postprocess/presence.py); share and inside are
    # computed from the stored integer counts
    m = fd.message_type.add(); m.name = "ZoneHit"
    _field(m, "index", 1, F.TYPE_INT32)
    _field(m, "name", 2, F.TYPE_STRING)
    _field(m, "pixels", 3, F.TYPE_UINT32)
    _field(m, "share", 4, F.TYPE_FLOAT)    # pixels / region pixels
    _field(m, "inside", 5, F.TYPE_BOOL)
    _field(m, "dwell", 6, F.TYPE_UINT32)   # 0 without has_tracks

    m = fd.message_type.add(); m.name = "RegionPresence"
    _field(m, "index", 1, F.TYPE_INT32)
    _field(m, "label", 2, F.TYPE_STRING)
    _field(m, "class_id", 3, F.TYPE_INT32)
    _field(m, "root", 4, F.TYPE_UINT32)
    _field(m, "pixels", 5, F.TYPE_UINT32)
    _field(m, "track_id", 6, F.TYPE_UINT32)
    _field(m, "age", 7, F.TYPE_UINT32)
    # the user zones with pixels > 0, index ascending
    _field(m, "zones", 8, F.TYPE_MESSAGE, F.LABEL_REPEATED, P + "ZoneHit")

    # the region x zone pixel overlap of the stream's latest frame
    m = fd.message_type.add(); m.name = "ZonePresence"
    _field(m, "stream_id", 1, F.TYPE_INT32)
    _field(m, "frame_id", 2, F.TYPE_INT64)
    _field(m, "timestamp", 3, F.TYPE_DOUBLE)
    _field(m, "width", 4, F.TYPE_INT32)    # crop region, model-resolution pixels
    _field(m, "height", 5, F.TYPE_INT32)
    _field(m, "model_width", 6, F.TYPE_INT32)
    _field(m, "model_height", 7, F.TYPE_INT32)
    _field(m, "regions", 8, F.TYPE_MESSAGE, F.LABEL_REPEATED, P + "RegionPresence")
    _field(m, "has_tracks", 9, F.TYPE_BOOL)   # the regions carry track_id, age and dwell
    _field(m, "min_share", 10, F.TYPE_FLOAT)  # q / 1024 of --presence_min_share

    m = fd.message_type.add(); m.name = "EventRequest"
    _field(m, "stream_id", 1, F.TYPE_INT32)
    _field(m, "after_seq", 2, F.TYPE_UINT64)
    _field(m, "max_events", 3, F.TYPE_INT32)   # 0 -> 1024
    _field(m, "zones", 4, F.TYPE_INT32, F.LABEL_REPEATED)  # zone indices to return; empty -> all, 0 = "frame"

    # one edge of a track's dwell in a zone (postprocess/events.py)
    m = fd.message_type.add(); m.name = "ZoneEvent"
    _field(m, "seq", 1, F.TYPE_UINT64)
    _field(m, "epoch", 2, F.TYPE_UINT32)
    _field(m, "kind", 3, F.TYPE_INT32)         # 1 ENTER, 2 LEAVE
    _field(m, "frame_id", 4, F.TYPE_INT64)
    _field(m, "timestamp", 5, F.TYPE_DOUBLE)
    _field(m, "zone", 6, F.TYPE_INT32)
    _field(m, "zone_name", 7, F.TYPE_STRING)
    _field(m, "track_id", 8, F.TYPE_UINT32)
    _field(m, "class_id", 9, F.TYPE_INT32)
    _field(m, "label", 10, F.TYPE_STRING)
    _field(m, "root", 11, F.TYPE_UINT32)
    _field(m, "track_edge", 12, F.TYPE_BOOL)
    _field(m, "pixels", 13, F.TYPE_UINT32)     # ENTER: region pixels inside the zone
    _field(m, "dwell", 14, F.TYPE_UINT32)      # LEAVE: frames it stayed

    # a stretch of the stream's event log
    m = fd.message_type.add(); m.name = "ZoneEvents"
    _field(m, "stream_id", 1, F.TYPE_INT32)
    _field(m, "events", 2, F.TYPE_MESSAGE, F.LABEL_REPEATED, P + "ZoneEvent")
    _field(m, "next_seq", 3, F.TYPE_UINT64)    # pass as after_seq next time
    _field(m, "lost", 4, F.TYPE_UINT64)
    _field(m, "truncated", 5, F.TYPE_UINT64)
    _field(m, "min_share", 6, F.TYPE_FLOAT)

    svc = fd.service.add()
    svc.name = "SemanticSegmentationV2"
    E = ".sem_seg_server.Empty"
    _method(svc, "GetStreamSegmentedObjects", P + "StreamRequest", P + "StreamSegmentedObjects")
    _method(svc, "ListStreams", E, P + "StreamList")
    _method(svc, "GetStats", E, P + "Stats")
    _method(svc, "Health", E, P + "HealthStatus")
    _method(svc, "GetSegmentationMask", P + "MaskRequest", P + "SegmentationMask")
    _method(svc, "GetClassRegions", P + "RegionRequest", P + "ClassRegions")
    _method(svc, "GetZoneOccupancy", P + "ZoneRequest", P + "ZoneOccupancy")
    _method(svc, "GetZonePresence", P + "PresenceRequest", P + "ZonePresence")
    _method(svc, "GetZoneEvents", P + "EventRequest", P + "ZoneEvents")
    return fd


HEALTH_SERVICE = "grpc.health.v1.Health"


def health_file_descriptor() -> descriptor_pb2.FileDescriptorProto:
    """The standard gRPC health-checking protocol (grpc/health/v1/health.proto),
    so stock probes (grpc_health_probe, load balancers, k8s) can query the server
    without grpcio-health-checking installed."""
    fd = descriptor_pb2.FileDescriptorProto()
    fd.name = "grpc/health/v1/health.proto"
    fd.package = "grpc.health.v1"
    fd.syntax = "proto3"
    m = fd.message_type.add(); m.name = "HealthCheckRequest"
    _field(m, "service", 1, F.TYPE_STRING)
    m = fd.message_type.add(); m.name = "HealthCheckResponse"
    e = m.enum_type.add(); e.name = "ServingStatus"
    for i, n in enumerate(["UNKNOWN", "SERVING", "NOT_SERVING", "SERVICE_UNKNOWN"]):
        v = e.value.add(); v.name = n; v.number = i
    _field(m, "status", 1, F.TYPE_ENUM,
           type_name=".grpc.health.v1.HealthCheckResponse.ServingStatus")
    svc = fd.service.add(); svc.name = "Health"
    _method(svc, "Check", ".grpc.health.v1.HealthCheckRequest", ".grpc.health.v1.HealthCheckResponse")
    w = _method(svc, "Watch", ".grpc.health.v1.HealthCheckRequest", ".grpc.health.v1.HealthCheckResponse")
    w.server_streaming = True
    return fd


POOL = descriptor_pool.DescriptorPool()
_V1_FD = POOL.Add(v1_file_descriptor())
_V2_FD = POOL.Add(v2_file_descriptor())
_HEALTH_FD = POOL.Add(health_file_descriptor())


def _cls(full_name: str):
    return message_factory.GetMessageClass(POOL.FindMessageTypeByName(full_name))


# ---- v1 (reference-compatible) -------------------------------------------
SegmentedObject = _cls("sem_seg_server.SegmentedObject")
Centroid = SegmentedObject.Centroid
SegmentedObjectData = _cls("sem_seg_server.SegmentedObjectData")
CameraResolution = _cls("sem_seg_server.CameraResolution")
Empty = _cls("sem_seg_server.Empty")

# ---- v2 (extension) --------------------------------------------------------
StreamRequest = _cls("sem_seg_server.v2.StreamRequest")
TaggedObject = _cls("sem_seg_server.v2.TaggedObject")
StreamSegmentedObjects = _cls("sem_seg_server.v2.StreamSegmentedObjects")
StreamInfo = _cls("sem_seg_server.v2.StreamInfo")
StreamList = _cls("sem_seg_server.v2.StreamList")
Stats = _cls("sem_seg_server.v2.Stats")
HealthStatus = _cls("sem_seg_server.v2.HealthStatus")
MaskRequest = _cls("sem_seg_server.v2.MaskRequest")
SegmentationMask = _cls("sem_seg_server.v2.SegmentationMask")
RegionRequest = _cls("sem_seg_server.v2.RegionRequest")
ClassRegion = _cls("sem_seg_server.v2.ClassRegion")
ClassRegions = _cls("sem_seg_server.v2.ClassRegions")
ZoneRequest = _cls("sem_seg_server.v2.ZoneRequest")
ZoneClass = _cls("sem_seg_server.v2.ZoneClass")
Zone = _cls("sem_seg_server.v2.Zone")
ZoneOccupancy = _cls("sem_seg_server.v2.ZoneOccupancy")
PresenceRequest = _cls("sem_seg_server.v2.PresenceRequest")
ZoneHit = _cls("sem_seg_server.v2.ZoneHit")
RegionPresence = _cls("sem_seg_server.v2.RegionPresence")
ZonePresence = _cls("sem_seg_server.v2.ZonePresence")
EventRequest = _cls("sem_seg_server.v2.EventRequest")
ZoneEvent = _cls("sem_seg_server.v2.ZoneEvent")
ZoneEvents = _cls("sem_seg_server.v2.ZoneEvents")

# ---- grpc.health.v1 ---------------------------------------------------------
HealthCheckRequest = _cls("grpc.health.v1.HealthCheckRequest")
HealthCheckResponse = _cls("grpc.health.v1.HealthCheckResponse")

V1_METHODS = {
    "GetSegmentedObjects": (Empty, SegmentedObjectData),
    "GetCameraResolution": (Empty, CameraResolution),
}
V2_METHODS = {
    "GetStreamSegmentedObjects": (StreamRequest, StreamSegmentedObjects),
    "ListStreams": (Empty, StreamList),
    "GetStats": (Empty, Stats),
    "Health": (Empty, HealthStatus),
    "GetSegmentationMask": (MaskRequest, SegmentationMask),
    "GetClassRegions": (RegionRequest, ClassRegions),
    "GetZoneOccupancy": (ZoneRequest, ZoneOccupancy),
    "GetZonePresence": (PresenceRequest, ZonePresence),
    "GetZoneEvents": (EventRequest, ZoneEvents),
}


def file_descriptor_set_bytes() -> bytes:
    """Serialized FileDescriptorSet of both files (for reflection/debugging)."""
    s = descriptor_pb2.FileDescriptorSet()
    s.file.add().CopyFrom(v1_file_descriptor())
    s.file.add().CopyFrom(v2_file_descriptor())
    s.file.add().CopyFrom(health_file_descriptor())
    return s.SerializeToString()
