"""The device class-region kernels (csrc/hip/class_regions.hip) against the definition
(``postprocess/regions.py`` ``encode``) on the inputs of tests/region_cases.py: every filling
of a 3 x 4 window at five places of the tile grid, thin / exact / ragged crops, the 16-bit
coordinate limit, the selection sort at its sizes, the statistics slots, and one workspace and
one out buffer reused across calls of different shapes and forms.
tests/test_region_cases_cpu.py holds the same inputs to a second oracle and asserts that each
case has the property it is listed for.

One comparator everywhere, ``run_and_compare``; every comparison is exact:

* every uint32 word of the out buffer equals the definition's row: header, records, and past
  the used words whatever the buffer held before the call (a sentinel, or an earlier call's
  words); so do the words of the buffer past the rows of this call;
* the workspace bytes past ``class_regions_workspace_bytes`` are what they were;
* the label plane and the confidence plane are what they were.

The workspace is prefilled with each of ``FILLS``: ``cnt[]`` carries a slot bit in bit 31 and
the statistics slots are reset per run, so no result may depend on what an earlier owner left.
"""
import numpy as np
import pytest
import torch

import region_cases as RC
from semantic_segmentation_server_amd.postprocess import regions as RG

pytestmark = pytest.mark.gpu

DEV = "cuda"
FILLS = (0x00, 0xFF, 0xA5)
WS_TAIL = 256
OUT_TAIL = 16


def _hip():
    from semantic_segmentation_server_amd.ops import hip_ops
    return hip_ops


class Buffers:
    """One out allocation and one workspace allocation; a call takes views of them."""

    def __init__(self, out_words, ws_bytes):
        self.out = torch.full((out_words + OUT_TAIL,), RC.SENT, dtype=torch.int32, device=DEV)
        self.ws = torch.zeros((ws_bytes + WS_TAIL,), dtype=torch.uint8, device=DEV)

    @classmethod
    def for_call(cls, B, crop_h, crop_w, K, with_conf):
        return cls(B * (4 + RG.words_per_region(with_conf) * K),
                   _hip().class_regions_workspace_bytes(B, crop_h, crop_w, with_conf))


def _mismatch(got, want):
    at = np.flatnonzero(got != want)[:8]
    return [(int(i), hex(int(got[i])), hex(int(want[i]))) for i in at]


def run_and_compare(bufs, labels, conf, want, *, crop_h, crop_w, classes, min_pixels, K, launch=None,
                    what=""):
    """THE comparator. ``labels`` [B, H, W] uint8 and ``conf`` (the same shape, or None: the
    6-word form) are numpy; ``want`` [B, 4 + 6|7 K] the definition's rows (what they hold past
    the used words does not matter). ``launch(lab, cf, out, ws)`` replaces the call (a graph
    replay). Returns the rows the device wrote."""
    hip = _hip()
    B, H, W = labels.shape
    with_conf = conf is not None
    rw = RG.words_per_region(with_conf)
    row = 4 + rw * K
    nb = hip.class_regions_workspace_bytes(B, crop_h, crop_w, with_conf)
    assert bufs.ws.numel() >= nb + WS_TAIL and bufs.out.numel() >= B * row + OUT_TAIL
    assert want.shape == (B, row)
    before = bufs.out.cpu().numpy().view(np.uint32).copy()
    tail = bufs.ws[nb:].clone()
    out = bufs.out[:B * row].view(B, row)
    if launch is None:
        lab = torch.from_numpy(np.array(labels)).to(DEV)
        cf = torch.from_numpy(np.array(conf)).to(DEV) if with_conf else None
        hip.class_regions(lab, out, bufs.ws, B=B, H=H, W=W, crop_h=crop_h, crop_w=crop_w,
                          classes=list(classes), min_pixels=min_pixels, K=K, **({"conf": cf} if with_conf else {}))
    else:
        lab, cf = launch(labels, conf, out, bufs.ws)
    torch.cuda.synchronize()
    got = bufs.out.cpu().numpy().view(np.uint32)
    expect = before.copy()
    rows = expect[:B * row].reshape(B, row)
    for b in range(B):
        used = RG.used_words(want[b], K, conf=with_conf)
        rows[b, :used] = want[b, :used]
    assert np.array_equal(got, expect), (what, with_conf, "out (index, got, want)", _mismatch(got, expect))
    assert torch.equal(bufs.ws[nb:], tail), (what, with_conf, "workspace written past its size")
    assert np.array_equal(lab.cpu().numpy(), labels), (what, "label plane changed")
    if with_conf:
        assert np.array_equal(cf.cpu().numpy(), conf), (what, "conf plane changed")
    return got[:B * row].reshape(B, row).copy()


def check_with_every_fill(labels, conf, want, geometry, what):
    """A fresh pair of buffers; the workspace (its tail too) prefilled with each byte of FILLS
    and the out buffer with the sentinel. Returns the rows of the last run."""
    B = labels.shape[0]
    bufs = Buffers.for_call(B, geometry["crop_h"], geometry["crop_w"], geometry["K"], conf is not None)
    rows = None
    for fill in FILLS:
        bufs.ws.fill_(fill)
        bufs.out.fill_(RC.SENT)
        rows = run_and_compare(bufs, labels, conf, want, what=(what, hex(fill)), **geometry)
    return rows


# ---------------------------------------------------------------- 1. exhaustive windows
WIN_GEOMETRY = dict(crop_h=RC.WIN_CROP[0], crop_w=RC.WIN_CROP[1], classes=RC.WIN_CLASSES, min_pixels=1,
                    K=RC.WIN_K)


@pytest.mark.parametrize("with_conf", [False, True], ids=["6w", "7w"])
@pytest.mark.parametrize("pos", sorted(RC.WIN_POS))
def test_every_filling_of_the_window(pos, with_conf):
    """All 4096 fillings at one position, 256 frames a launch, against the flood fill on the
    twelve cells (tests/test_region_cases_cpu.py holds that to the definition)."""
    for j in range(RC.WIN_BATCHES):
        labels, conf = RC.window_batch(pos, j)
        check_with_every_fill(labels, conf if with_conf else None, RC.window_want(pos, j, with_conf),
                              WIN_GEOMETRY, ("window", pos, j))


# ---------------------------------------------------------------- 2 - 5. the case table
CASE_PARAMS = [pytest.param(c.name, f, id=f"{c.name}-{'7w' if f else '6w'}") for c in RC.CASES for f in c.forms]


@pytest.mark.parametrize("name,with_conf", CASE_PARAMS)
def test_case(name, with_conf):
    case = RC.BY_NAME[name]
    b = RC.built(case)
    want = RC.want(case, with_conf)
    rows = check_with_every_fill(b.labels, b.conf if with_conf else None, want, b.geometry, name)
    assert np.array_equal(rows[:, :4], want[:, :4])


# ---------------------------------------------------------------- 6. one workspace, one out buffer
REUSE = ("select-full-K256", "shape-%dx%d:1" % RC.SHAPES[8], "giant", "shape-7x1", "stats-256-slots",
         "stats-conf-runs")


def _call_inputs(key):
    """(labels, conf, geometry) of a step of the reuse sequences: a case of the table, one frame
    of a case (``name:frame``), or one region over a 3 x 3-tile ragged crop."""
    if key == "giant":
        ch, cw = 2 * RC.TH + 9, 3 * RC.TW + 1
        labels = np.full((2, ch + 4, cw + 4), 5, np.uint8)
        conf = np.random.default_rng(9).integers(0, 256, labels.shape, dtype=np.uint8)
        return labels, conf, dict(crop_h=ch, crop_w=cw, classes=(5,), min_pixels=2, K=16)
    name, _, frame = key.partition(":")
    b = RC.built(RC.BY_NAME[name])
    if frame:
        return b.labels[int(frame):int(frame) + 1], b.conf[int(frame):int(frame) + 1], b.geometry
    return b.labels, b.conf, b.geometry


_REUSE_WANT = {}


def _call_want(key, with_conf):
    if (key, with_conf) not in _REUSE_WANT:
        labels, conf, g = _call_inputs(key)
        w = RC.definition_rows(labels, conf, g["crop_h"], g["crop_w"], g["classes"], g["min_pixels"], g["K"],
                               with_conf)
        w.setflags(write=False)
        _REUSE_WANT[(key, with_conf)] = w
    return _REUSE_WANT[(key, with_conf)]


def _largest(keys):
    hip = _hip()
    out_words = ws_bytes = 0
    for key in keys:
        labels, _, g = _call_inputs(key)
        B = labels.shape[0]
        out_words = max(out_words, B * (4 + 7 * g["K"]))
        ws_bytes = max(ws_bytes, hip.class_regions_workspace_bytes(B, g["crop_h"], g["crop_w"], True))
    return Buffers(out_words, ws_bytes)


def _step(bufs, key, with_conf):
    labels, conf, g = _call_inputs(key)
    return run_and_compare(bufs, labels, conf if with_conf else None, _call_want(key, with_conf),
                           what=("reuse", key), **g)


def test_reuse_steps_are_what_they_are_listed_for():
    """The empty frame has no region; the giant frames one each; the sequence starts at the
    largest candidate list, passes the smallest crop and the largest, and ends at 5 x 4 tiles."""
    assert _call_want(REUSE[1], False)[0, 0] == 0
    assert _call_want("giant", False)[:, 0].tolist() == [1, 1]
    assert _call_want(REUSE[0], False)[0, 0] == RC.CAND
    sizes = [_call_inputs(k)[2]["crop_h"] * _call_inputs(k)[2]["crop_w"] for k in REUSE]
    assert max(sizes) == sizes[4] and sizes[3] == 7 and sizes[5] == RC.STAT_CROP[0] * RC.STAT_CROP[1]


@pytest.mark.parametrize("fill", FILLS, ids=[hex(f) for f in FILLS])
@pytest.mark.parametrize("with_conf", [False, True], ids=["6w", "7w"])
def test_one_workspace_and_out_buffer_across_shapes(with_conf, fill):
    """REGION_CANDIDATES singletons, an empty frame, one giant region (two frames), a 7 x 1
    crop, the 9 x 8-tile crop with 256 regions, the 5 x 4-tile crop: nothing is refilled or
    reallocated between the calls, so every call meets the parents, counts, slot bits, slots and
    out words of a larger, differently shaped earlier one."""
    bufs = _largest(REUSE)
    bufs.ws.fill_(fill)
    for key in REUSE:
        _step(bufs, key, with_conf)


@pytest.mark.parametrize("fill", FILLS, ids=[hex(f) for f in FILLS])
def test_forms_alternate_on_one_workspace_and_repeat(fill):
    """7-word, 6-word, 7-word calls on the same buffers (the CONF sums live behind the
    workspace of the 6-word form), on two geometries; then one call twice: identical rows."""
    bufs = _largest(REUSE)
    bufs.ws.fill_(fill)
    for key in ("stats-conf-runs", "select-full-K256", "stats-conf-runs"):
        for with_conf in (True, False, True):
            _step(bufs, key, with_conf)
    first = _step(bufs, "stats-256-slots", True)
    again = _step(bufs, "stats-256-slots", True)
    assert first.tobytes() == again.tobytes()


@pytest.mark.parametrize("with_conf", [False, True], ids=["6w", "7w"])
def test_window_batch_captured_in_a_graph_and_replayed_on_new_planes(with_conf):
    """As test_regions_gpu.py::test_captured_in_a_graph_and_replayed_on_new_labels, with three
    batches of the corner window: the replay reads the planes it was captured on."""
    hip = _hip()
    H, W = RC.WIN_MAP
    B = RC.WIN_BATCH
    g = WIN_GEOMETRY
    bufs = Buffers.for_call(B, g["crop_h"], g["crop_w"], g["K"], with_conf)
    bufs.ws.fill_(FILLS[2])
    lab = torch.zeros((B, H, W), dtype=torch.uint8, device=DEV)
    cf = torch.zeros_like(lab) if with_conf else None
    out = bufs.out[:B * (4 + RG.words_per_region(with_conf) * g["K"])].view(B, -1)

    def call():
        hip.class_regions(lab, out, bufs.ws, B=B, H=H, W=W, crop_h=g["crop_h"], crop_w=g["crop_w"],
                          classes=list(g["classes"]), min_pixels=g["min_pixels"], K=g["K"],
                          **({"conf": cf} if with_conf else {}))

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        call()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()

    def replay(labels, conf, out_view, ws):
        assert out_view.data_ptr() == out.data_ptr() and ws.data_ptr() == bufs.ws.data_ptr()
        lab.copy_(torch.from_numpy(labels))
        if with_conf:
            cf.copy_(torch.from_numpy(conf))
        graph.replay()
        return lab, cf

    for j in (0, 7, RC.WIN_BATCHES - 1):
        labels, conf = RC.window_batch("d", j)
        bufs.out.fill_(RC.SENT)
        run_and_compare(bufs, labels, conf if with_conf else None, RC.window_want("d", j, with_conf),
                        launch=replay, what=("graph", j), **g)
