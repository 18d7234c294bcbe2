"""Captured steps of the engine, one class per capture form: the hipGraphs of one frame buffer
and the static outputs they write (``labels``; ``post``: packed records or None; ``mask``:
--serve_masks run words or None; ``regions``: --serve_regions region words or None (two words a
record wider with --track_regions, whose per-stream state lives in the engine's one
DevicePostprocess: the post-processing graphs of all slots advance it in replay order); ``conf``: the
--serve_confidence plane of ``labels``, which the post-processing graph reads, or None;
``zones``: --serve_zones zone words, or None; ``presence``: --serve_presence presence words,
written by the last kernels of the post-processing chain (their dwell state lives beside the
track state), or None; ``events``: --serve_events event words, written by the kernels that then
end the chain, or None). With --stable_labels the first launch of the post-processing chain
rewrites ``labels`` (and ``conf``) in place with the stabilised planes, whose per-stream state
lives there too: after the post-processing they are what the step hands out. With
--smooth_labels the spatial filter is launched before that, into scratch planes of the
DevicePostprocess, and the same holds: ``labels`` (and ``conf``) end up smoothed.
``replay()`` issues that form's replays, waits and event records; after ``consumed`` the buffer
may be refilled (None: the model ran on the caller's stream).

With a raw pixel format (``eng.frame_channels == 2``) the frame buffer holds packed 4:2:2 bytes
and every step owns ``bgr``, the BGR frames its model reads: the conversion is the first kernel
of the step's model graph, on the model's stream. ``bgr`` is None with BGR ingest (no kernel).
"""
from __future__ import annotations

import torch

from ..utils import fast_cuda


def capture(eng, frames: torch.Tensor, slot: int = None):
    """The step that runs ``eng`` on ``frames``; ``slot``: the index of a buffer declared
    with ``bind_inputs`` (None: the engine's static input, always one whole graph)."""
    dev = eng.device
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        for _ in range(2):  # warm up allocator / lazy init outside capture
            eng._step_outputs(frames)
    torch.cuda.current_stream(dev).wait_stream(s)
    if slot is None or not eng._split:
        return WholeStep(eng, frames)
    if eng.slot_parallel:
        return SlotStep(eng, frames, slot)
    B, P = frames.shape[0], eng.model_parts if eng._hip_model is not None else 1
    if P > 1 and B % P == 0 and B >= 2 * P:
        return PartsStep(eng, frames, P)
    return SplitStep(eng, frames)


def _graph(fn):
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = fn()
    return g, out


class WholeStep:
    """One graph, model + post-processing (+ masks, + regions), on the caller's stream."""

    def __init__(self, eng, frames):
        self.frames, self.consumed = frames, None
        self.bgr = bgr = eng.bgr_buffer(frames)
        self.graph, (self.labels, self.post, self.mask, self.regions, self.conf) = _graph(
            lambda: eng._step_all(frames, bgr))
        self.zones = eng._step_zones  # --serve_zones: the zone words the graph writes, or None
        self.presence = eng._step_presence  # --serve_presence: the same
        self.events = eng._step_events  # --serve_events: the same

    def replay(self) -> None:
        self.graph.replay()


class SplitStep:
    """The model graph on the caller's stream, the post-processing graph (records, then the
    run-length masks, then the class regions: one chain) on the engine's ``result_stream``."""

    def __init__(self, eng, frames, part: int = 0):
        hm, dev = eng._hip_model, eng.device
        self.frames, self.consumed, self.device = frames, None, dev
        # the model writes the step's own label maps
        self.labels = lab = torch.empty((frames.shape[0], eng.H, eng.W), dtype=torch.uint8, device=dev)
        self.bgr = bgr = eng.bgr_buffer(frames)  # raw ingest: converted into, then read by segment
        # ... and, with --serve_confidence, the step's own confidence plane
        self.conf = cf = torch.empty_like(lab) if eng.serve_confidence else None

        def segment():
            return hm.segment(eng.to_bgr(frames, out=bgr), eng.lut_x, eng.lut_y, out=lab, part=part,
                              conf_out=cf)

        def infer():  # no plan (the torch backend): copied into the step's planes
            labels, conf = eng._infer(frames, bgr)
            lab.copy_(labels)
            if cf is not None:
                cf.copy_(conf)

        if eng.slot_parallel:  # SlotStep: this slot's plan copy is built outside capture
            segment()
            torch.cuda.synchronize(dev)
        if hm is not None:
            self.model, _ = _graph(segment)
        else:
            self.model, _ = _graph(infer)
        self.post_graph, (self.post, self.mask, self.regions) = _graph(lambda: eng._post_and_mask(lab, conf=cf))
        self.zones = eng.device_zones()  # --serve_zones, or None
        self.presence = eng.device_presence()  # --serve_presence: after the zones in the chain, or None
        self.events = eng.device_events()  # --serve_events: the last kernels of the chain, or None
        self.rs, self.post_done = eng.result_stream, torch.cuda.Event()

    def replay(self) -> None:
        cur = torch.cuda.current_stream(self.device)
        cur.wait_event(self.post_done)  # this step's previous post-processing read `labels`
        self.model.replay()
        ready = torch.cuda.Event()
        ready.record(cur)
        rs = self.rs
        rs.wait_event(ready)
        with torch.cuda.stream(rs):
            self.post_graph.replay()
        self.post_done.record(rs)


class SlotStep(SplitStep):
    """Slot-parallel: the model graph on the staging slot's own stream, with its own plan copy."""
    # the previous step (other slot, other stream, other plan copy) may still be running.
    # Per-step host work kept to C calls (utils/fast_cuda.py; the slot's events are reused:
    # a slot's next step is at least one step later)

    def __init__(self, eng, frames, slot: int):
        super().__init__(eng, frames, part=slot)
        self.ms, self.h2d_on_slot, self.device_index = eng.slot_streams[slot], eng.h2d_on_slot, eng.device_index
        self.fork, self.ready = torch.cuda.Event(), torch.cuda.Event()
        self.consumed = self.ready  # the staging slot may be refilled after this

    def replay(self) -> None:
        ms, rs, post_done, ready = self.ms, self.rs, self.post_done, self.ready
        if self.h2d_on_slot:  # frames were uploaded on ms itself
            ms.wait_event(post_done)
        else:
            cur = fast_cuda.current_stream(self.device_index)
            cur.wait_event(post_done)  # this slot's previous post-processing read `labels`
            self.fork.record(cur)  # cur waited for this slot's frames (H2D)
            ms.wait_event(self.fork)
        with fast_cuda.StreamSwitch(ms):
            self.model.replay()
        ready.record(ms)
        rs.wait_event(ready)
        with fast_cuda.StreamSwitch(rs):
            self.post_graph.replay()
        post_done.record(rs)


class PartsStep:
    """P sub-batch model graphs on P streams (the caller's and the engine's ``model_streams``),
    each part's post-processing graph on ``result_stream`` as soon as its labels exist."""
    # the latency-bound kernels of one part fill the others' tails

    def __init__(self, eng, frames, P: int):
        hm, dev, B = eng._hip_model, eng.device, frames.shape[0]
        self.frames, self.consumed, self.device = frames, None, dev
        sls = [slice(i * (B // P), (i + 1) * (B // P)) for i in range(P)]
        self.labels = lab = torch.empty((B, eng.H, eng.W), dtype=torch.uint8, device=dev)
        self.bgr = bgr = eng.bgr_buffer(frames)  # raw ingest: each part converts its own slice
        self.post = post = torch.zeros((B, 1 + 5 * eng.cfg.max_segments), dtype=torch.float32, device=dev)
        self.mask = mask = torch.zeros((B, 4 + eng.mask_cap), dtype=torch.int32,
                                       device=dev) if eng.mask_cap else None
        self.regions = reg = torch.zeros((B, 4 + eng.region_words * eng.region_cap), dtype=torch.int32,
                                         device=dev) if eng.region_cap else None
        self.conf = cf = torch.empty_like(lab) if eng.serve_confidence else None
        self.zones = zn = None
        if eng.zone_rows:
            from ..postprocess import zones as ZN
            self.zones = zn = torch.zeros((B, ZN.frame_words(eng.zone_rows, eng.zone_classes, eng.zone_conf)),
                                          dtype=torch.int32, device=dev)
        self.presence = pr = None
        if eng.presence_rows:
            self.presence = pr = torch.zeros((B, 4 + eng.presence_unit * eng.region_cap), dtype=torch.int32,
                                             device=dev)
        self.events = evs = None
        if eng.event_cap:
            self.events = evs = torch.zeros((B, 4 + 4 * eng.event_cap), dtype=torch.int32, device=dev)
        parts = [(lambda i=i, sl=sl: hm.segment(eng.to_bgr(frames[sl], out=bgr[sl] if bgr is not None else None),
                                                eng.lut_x, eng.lut_y, out=lab[sl], part=i,
                                                conf_out=cf[sl] if cf is not None else None),
                  lambda sl=sl: eng._device_post(lab[sl], out=post[sl],
                                                 mask_out=mask[sl] if mask is not None else None,
                                                 region_out=reg[sl] if reg is not None else None,
                                                 conf=cf[sl] if cf is not None else None,
                                                 zone_out=zn[sl] if zn is not None else None,
                                                 presence_out=pr[sl] if pr is not None else None,
                                                 event_out=evs[sl] if evs is not None else None))
                 for i, sl in enumerate(sls)]  # per part: (model, records)
        for run in [m for m, _ in parts] + [r for _, r in parts]:  # warm-up outside capture
            run()
        torch.cuda.synchronize(dev)
        graphs = [(_graph(m)[0], _graph(r)[0]) for m, r in parts]  # captured in that order
        self.models, self.posts = zip(*graphs)
        while len(eng.model_streams) < P - 1:
            eng.model_streams.append(torch.cuda.Stream(dev))
        self.side, self.rs, self.post_done = eng.model_streams[:P - 1], eng.result_stream, torch.cuda.Event()

    def replay(self) -> None:
        cur = torch.cuda.current_stream(self.device)
        cur.wait_event(self.post_done)  # this step's previous post-processing read `labels`
        rs = self.rs
        fork = torch.cuda.Event()
        fork.record(cur)
        ready = []
        for st, g in zip([cur] + self.side, self.models):
            if st is not cur:
                st.wait_event(fork)
            with torch.cuda.stream(st):
                g.replay()
            ev = torch.cuda.Event()
            ev.record(st)
            ready.append(ev)
        for ev in ready[1:]:  # cur joins every part: the staging slot is free only after
            cur.wait_event(ev)  # all of them read it
        with torch.cuda.stream(rs):
            for ev, gp in zip(ready, self.posts):
                rs.wait_event(ev)
                gp.replay()
        self.post_done.record(rs)
