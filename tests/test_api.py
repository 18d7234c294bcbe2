"""T1/T5: wire compatibility of the v1 proto and servicer semantics.

The expected bytes are hand-encoded from the reference schema
(sem_seg_server.proto:14-50: label=1 string, score=2 float, area=3 float,
centroid=4 message{cx=1 float, cy=2 float}; data=1 repeated; width=1/height=2 int32).
"""
import os
import struct

import grpc
import numpy as np
import pytest

from semantic_segmentation_server_amd.api import proto as P
from semantic_segmentation_server_amd.api import service as S
from semantic_segmentation_server_amd.labels import load_labels
from semantic_segmentation_server_amd.runtime.results import RECORD_DTYPE, ResultBuffer, ResultHub, make_records

REF_DESCRIPTOR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                              "sem_seg_server_v1_descriptor.json")


def _f32(tag, v):
    return bytes([tag]) + struct.pack("<f", v)


def test_segmented_object_wire_bytes():
    o = P.SegmentedObject(label="person", score=0.5, area=0.25, centroid=P.Centroid(cx=0.5, cy=0.75))
    cen = _f32(0x0D, 0.5) + _f32(0x15, 0.75)
    exp = b"\x0a\x06person" + _f32(0x15, 0.5) + _f32(0x1D, 0.25) + b"\x22" + bytes([len(cen)]) + cen
    assert o.SerializeToString() == exp
    assert P.SegmentedObject.FromString(exp) == o


def test_padding_entry_serializes_empty():
    d = P.SegmentedObjectData(data=[P.SegmentedObject()])
    assert d.SerializeToString() == b"\x0a\x00"
    assert not d.data[0].HasField("centroid")


def test_camera_resolution_wire():
    assert P.CameraResolution(width=640, height=480).SerializeToString() == b"\x08\x80\x05\x10\xe0\x03"
    assert P.Empty().SerializeToString() == b""


def test_service_names():
    fd = P.POOL.FindFileByName("sem_seg_server.proto")
    svc = fd.services_by_name["SemanticSegmentation"]
    assert svc.full_name == "sem_seg_server.SemanticSegmentation"
    assert [m.name for m in svc.methods] == ["GetSegmentedObjects", "GetCameraResolution"]
    assert svc.methods_by_name["GetSegmentedObjects"].output_type.full_name == \
        "sem_seg_server.SegmentedObjectData"


def test_descriptor_matches_reference_serialized_descriptor():
    """Compare every message/field/method with the reference's FileDescriptorProto, as
    recorded in tests/golden (package; per message the sorted (name, number, type, label,
    type_name) of its fields; per method (name, input type, output type))."""
    import json
    with open(REF_DESCRIPTOR) as f:
        ref = json.load(f)
    ours = P.v1_file_descriptor()
    assert ref["package"] == ours.package

    def msgs(fd):
        out = {}

        def walk(m, prefix):
            out[prefix + m.name] = sorted((f.name, f.number, f.type, f.label, f.type_name) for f in m.field)
            for n in m.nested_type:
                walk(n, prefix + m.name + ".")
        for m in fd.message_type:
            walk(m, "")
        return out
    assert len(ref["messages"]) == 5
    assert {k: [tuple(f) for f in v] for k, v in ref["messages"].items()} == msgs(ours)
    rs = {tuple(m) for m in ref["methods"]}
    os_ = {(m.name, m.input_type, m.output_type) for s in ours.service for m in s.method}
    assert len(rs) == 2 and rs == os_


def _recs(labels):
    return make_records([(l, 0.9, 0.1, 0.2, 0.3, 0, i, 0.0) for i, l in enumerate(labels)])


def test_buffer_lifo_and_bound():
    b = ResultBuffer(maxlen=3)
    b.push_frame(_recs([1, 2]))   # frame 1 contours 0,1
    b.push_frame(_recs([3, 4]))   # frame 2
    assert b.drops == 1            # oldest (label 1) dropped
    got = [int(r["label"]) for r in b.pop(5)]
    assert got == [4, 3, 2]        # newest frame's last contour first
    assert b.pop(1) == []


def test_v1_get_segmented_objects_pads_and_pops():
    hub = ResultHub(1)
    labels = load_labels()
    sv = S.SemanticSegmentationServicer(hub, labels, num_detections=3, camera_res=(640, 480))
    hub.push_records(_recs([15, 7]))
    r = sv.GetSegmentedObjects(P.Empty(), None)
    assert len(r.data) == 3
    assert [d.label for d in r.data] == ["car", "person", ""]
    assert r.data[0].centroid.cx == pytest.approx(0.2)
    assert not r.data[2].HasField("centroid")
    r2 = sv.GetSegmentedObjects(P.Empty(), None)
    assert [d.label for d in r2.data] == ["", "", ""]
    assert sv.GetCameraResolution(P.Empty(), None).width == 640


def test_unknown_label_is_stringified():
    hub = ResultHub(1)
    sv = S.SemanticSegmentationServicer(hub, {0: "background"}, num_detections=1)
    hub.push_records(_recs([42]))
    assert sv.GetSegmentedObjects(P.Empty(), None).data[0].label == "42"


def test_grpc_loopback_v1_and_v2():
    hub = ResultHub(2)
    labels = load_labels()
    server, port = S.make_server(4, 0, "127.0.0.1")
    S.add_v1_servicer(S.SemanticSegmentationServicer(hub, labels, 3, (640, 480)), server)
    S.add_v2_servicer(S.SemanticSegmentationV2Servicer(
        hub, labels, 3, [dict(stream_id=1, width=320, height=240, rank=0, source="synthetic")]),
        server)
    server.start()
    try:
        hub.push_records(_recs([15]))
        r = make_records([(7, 1.0, 0.5, 0.5, 0.5, 1, 99, 123.0)])
        hub.push_records(r)
        with grpc.insecure_channel(f"127.0.0.1:{port}") as ch:
            st = S.SemanticSegmentationStub(ch)
            assert st.GetCameraResolution(P.Empty()).height == 480
            d = st.GetSegmentedObjects(P.Empty())
            assert [x.label for x in d.data] == ["person", "", ""]
            v2 = S.SemanticSegmentationV2Stub(ch)
            t = v2.GetStreamSegmentedObjects(P.StreamRequest(stream_id=1, max_objects=2, pad=True))
            assert len(t.data) == 2 and t.data[0].frame_id == 99 and t.data[0].object.label == "car"
            assert v2.ListStreams(P.Empty()).streams[0].width == 320
            assert v2.Health(P.Empty()).serving
            assert v2.GetStats(P.Empty()).buffer_depth == 0
    finally:
        server.stop(0)


def test_v2_bounds_client_input():
    """max_objects is clamped, unknown stream ids are NOT_FOUND and never
    allocate a buffer."""
    hub = ResultHub(1, maxlen=8)
    sv = S.SemanticSegmentationV2Servicer(hub, load_labels(), 3)
    hub.push_records(_recs([15, 7]))

    class Ctx:
        code = None

        def set_code(self, c):
            self.code = c

        def set_details(self, d):
            self.details = d
    ctx = Ctx()
    r = sv.GetStreamSegmentedObjects(P.StreamRequest(stream_id=0, max_objects=2 ** 31 - 1, pad=True), ctx)
    assert len(r.data) == 8 and ctx.code is None          # clamped to the buffer capacity
    assert [d.object.label for d in r.data[:2]] == ["car", "person"]
    r = sv.GetStreamSegmentedObjects(P.StreamRequest(stream_id=0, max_objects=-5, pad=True), ctx)
    assert len(r.data) == 0
    r = sv.GetStreamSegmentedObjects(P.StreamRequest(stream_id=12345, max_objects=3, pad=True), ctx)
    assert ctx.code == grpc.StatusCode.NOT_FOUND and len(r.data) == 0
    assert set(hub.buffers) == {0}


def test_grpc_health_v1():
    state = {"ok": True}
    server, port = S.make_server(4, 0, "127.0.0.1")
    S.add_health_servicer(S.HealthServicer(lambda service: state["ok"], watch_period=0.05), server)
    server.start()
    try:
        with grpc.insecure_channel(f"127.0.0.1:{port}") as ch:
            h = S.HealthStub(ch)
            R = P.HealthCheckResponse
            assert h.Check(P.HealthCheckRequest(service="")).status == R.SERVING
            assert h.Check(P.HealthCheckRequest(service=P.V1_SERVICE)).status == R.SERVING
            with pytest.raises(grpc.RpcError) as ei:
                h.Check(P.HealthCheckRequest(service="nope"))
            assert ei.value.code() == grpc.StatusCode.NOT_FOUND
            state["ok"] = False
            assert h.Check(P.HealthCheckRequest()).status == R.NOT_SERVING
            it = h.Watch(P.HealthCheckRequest())
            assert next(it).status == R.NOT_SERVING
            state["ok"] = True
            assert next(it).status == R.SERVING
            it.cancel()
    finally:
        server.stop(0)


def test_health_descriptor_matches_standard_wire_format():
    # grpc.health.v1.HealthCheckResponse{status = SERVING(1)} -> 08 01
    assert P.HealthCheckResponse(status=1).SerializeToString() == b"\x08\x01"
    assert P.HealthCheckRequest(service="x").SerializeToString() == b"\x0a\x01x"
