"""Smooth labels on the host: the numpy implementation (postprocess/smooth.py ``apply``) against
the definition spelled out pixel by pixel (``apply_slow``), every three-label 3 x 3 pattern, the
confidence rule, the configuration refusals, and the CPU engine, whose masks must see the
smoothed maps -- ahead of the stabilisation when both are on. All integer, no tolerance."""
import numpy as np
import pytest
import torch

from semantic_segmentation_server_amd import config as C
from semantic_segmentation_server_amd.postprocess import mask_rle as MR
from semantic_segmentation_server_amd.postprocess import smooth as SM
from semantic_segmentation_server_amd.postprocess import stable as SB

import smooth_cases as SC


def _same(got, want):
    assert np.array_equal(got[0], want[0])
    assert (got[1] is None) == (want[1] is None)
    assert got[1] is None or np.array_equal(got[1], want[1])


@pytest.mark.parametrize("R", [1, 2, 3])
@pytest.mark.parametrize("gi", range(len(SC.CPU_GEOMETRIES)))
def test_apply_equals_the_pixel_by_pixel_definition(gi, R):
    H, W, ch, cw = SC.CPU_GEOMETRIES[gi]
    lab, codes = SC.random_maps(10 * gi + R, 3, H, W)
    lab0, codes0 = lab.copy(), codes.copy()
    want = SM.apply_slow(lab, codes, cw, ch, R)
    got = SM.apply(lab, codes, cw, ch, R)
    _same(got, want)
    _same(SM.apply(lab, None, cw, ch, R), (want[0], None))
    assert np.array_equal(lab, lab0) and np.array_equal(codes, codes0)  # the inputs are not written
    pad = np.ones((H, W), bool)
    pad[:ch, :cw] = False
    assert np.array_equal(got[0][:, pad], lab[:, pad]) and np.array_equal(got[1][:, pad], codes[:, pad])
    assert (got[0] != lab).any() or ch * cw == 1  # a 1 x 1 crop has nothing to outvote


def test_every_three_label_3x3_pattern():
    lab, codes = SC.exhaustive()
    assert lab.shape == (19683, 5, 6)
    want_c, kept, kept_tie, changed_tie = SC.exhaustive_centres()
    # from the definition alone: the inputs reach every rule
    assert int(kept.sum()) == 11811 and int(kept_tie.sum()) == 3360
    assert int((~kept).sum()) == 7872 and int(changed_tie.sum()) == 210
    got = SM.apply(lab, codes, 3, 3, 1)
    _same(got, SM.apply_slow(lab, codes, 3, 3, 1))
    assert np.array_equal(got[0][:, 1, 1], want_c)
    assert np.array_equal(got[0][:, 1, 1] == lab[:, 1, 1], kept)
    assert (got[0][:, 3:] == 9).all() and (got[0][:, :, 3:] == 9).all()
    assert np.array_equal(got[1][:, 3:], codes[:, 3:]) and np.array_equal(got[1][:, :, 3:], codes[:, :, 3:])


def test_conf_rule_floor_mean_of_the_winning_voters():
    lab = np.array([[[4, 4, 9, 0],
                     [4, 7, 9, 0],
                     [9, 9, 9, 0]]], np.uint8)
    codes = np.array([[[10, 20, 31, 1],
                       [30, 99, 41, 2],
                       [50, 60, 72, 3]]], np.uint8)
    out, cout = SM.apply(lab, codes, 3, 3, 1)  # the last column is pad
    # centre: 9 has five votes of nine; its voters' codes are 31, 41, 50, 60, 72 -> floor(254 / 5)
    assert out[0, 1, 1] == 9 and cout[0, 1, 1] == 254 // 5 == 50
    # (0, 0): window 4, 4, 4, 7 -- unchanged, keeps its code
    assert out[0, 0, 0] == 4 and cout[0, 0, 0] == 10
    # (0, 1): window 4 4 9 / 4 7 9 -> 4 stays; (1, 0): 4 4 / 4 7 / 9 9 -> 4 stays
    assert out[0, 0, 1] == 4 and cout[0, 0, 1] == 20 and out[0, 1, 0] == 4 and cout[0, 1, 0] == 30
    unchanged = out == lab
    assert np.array_equal(cout[unchanged], codes[unchanged])
    assert np.array_equal(out[:, :, 3], lab[:, :, 3]) and np.array_equal(cout[:, :, 3], codes[:, :, 3])
    _same((out, cout), SM.apply_slow(lab, codes, 3, 3, 1))
    out2, none = SM.apply(lab, None, 3, 3, 1)
    assert none is None and np.array_equal(out2, out)
    assert SM.apply_slow(lab, None, 3, 3, 1)[1] is None
    # the smallest label wins a tie the centre is not part of; 255 is a label like any other
    tie = np.array([[[255, 255, 3], [8, 200, 3], [8, 1, 2]]], np.uint8)
    assert SM.apply(tie, None, 3, 3, 1)[0][0, 1, 1] == 3
    assert SM.apply(np.array([[[255, 255, 3], [255, 200, 3], [8, 1, 2]]], np.uint8), None, 3, 3, 1)[0][0, 1, 1] == 255


def test_check_params_and_shapes():
    for R in (1, 2, 3):
        SM.check_params(R)
    for R in (0, 4, -1):
        with pytest.raises(ValueError, match="--smooth_labels"):
            SM.check_params(R)
    lab = np.zeros((1, 4, 4), np.uint8)
    with pytest.raises(ValueError, match="crop"):
        SM.apply(lab, None, 5, 4, 1)
    with pytest.raises(ValueError, match="conf"):
        SM.apply(lab, np.zeros((1, 4, 5), np.uint8), 4, 4, 1)
    with pytest.raises(ValueError, match="labels"):
        SM.apply(lab.astype(np.int32), None, 4, 4, 1)


# ---- configuration and engine -------------------------------------------------------------------

def _cfg(**kw):
    base = dict(backend="torch", device="cpu", input_size=129, batch=1, port=0, host="127.0.0.1",
                min_area_ratio=0.0005, fps_limit=200.0, log_level="WARNING")
    base.update(kw)
    return C.Config(**base)


def test_cli_flag_and_refusals():
    from semantic_segmentation_server_amd.runtime.engine import Engine
    assert C.parse([]).smooth_labels == 0
    for R in (1, 2, 3):
        assert C.parse(["--smooth_labels", str(R)]).smooth_labels == R
    for bad in ("4", "-1"):
        with pytest.raises(ValueError, match="--smooth_labels"):
            C.parse(["--smooth_labels", bad])
    with pytest.raises(ValueError, match="--smooth_labels 4 outside 1 .. 3"):
        C.Config(smooth_labels=4)
    off = Engine(_cfg(input_size=65))
    assert off.smooth_radius == 0
    on = Engine(_cfg(input_size=65, smooth_labels=2, streams=2))  # stateless: any stream layout
    assert on.smooth_radius == 2 and on.stable_frames == 0


def _engine_run(seq, **kw):
    """The CPU engine over planted label maps (its model's output replaced by ``seq``): the
    engine and, per step, the served run words."""
    from semantic_segmentation_server_amd.runtime.engine import Engine
    eng = Engine(_cfg(serve_masks=True, **kw))
    maps = iter(seq)
    eng._infer = lambda frames, bgr=None: (torch.from_numpy(next(maps).copy())[None], None)
    frame = np.zeros((1, 120, 160, 3), np.uint8)
    out = []
    for k in range(len(seq)):
        eng.step(frame, [k], [0.0], 0)
        out.append(eng.masks[0].copy())
    return eng, out


def _same_words(got, want):
    u = MR.used_words(want)
    assert np.array_equal(got[:u], want[:u])


def test_cpu_engine_serves_the_smoothed_maps_ahead_of_the_stabilisation():
    raw, _ = SC.speckled(31, 4, 129, 129, block=16)
    eng, got = _engine_run(list(raw), smooth_labels=1)
    cw, ch = eng.crop_w, eng.crop_h
    assert ch < 129 and cw == 129  # a letterboxed crop: pad rows exist
    sm, _ = SM.apply(raw, None, cw, ch, 1)
    assert (sm != raw).any()
    for k in range(4):
        _same_words(got[k], MR.encode(sm[k], cw, ch, eng.mask_cap))
        assert np.array_equal(MR.decode(got[k]), sm[k, :ch, :cw])
    # with --stable_labels as well: smoothing first, then the stabilisers, over four frames
    eng, got = _engine_run(list(raw), smooth_labels=1, stable_labels=3)
    st = SB.Stabilizers(3)
    seen = []
    for k in range(4):
        lab, _ = st.step(sm[k:k + 1], None, cw, ch, [0])
        seen.append(lab[0])
        _same_words(got[k], MR.encode(lab[0], cw, ch, eng.mask_cap))
    assert (seen[3] != sm[3]).any()  # the stabilisation did hold something back
    # flag off: the raw maps
    eng, got = _engine_run(list(raw[:1]))
    assert np.array_equal(MR.decode(got[0]), raw[0, :ch, :cw])


def test_server_on_cpu_serves_a_mask_of_the_smoothed_map(monkeypatch):
    import grpc
    from semantic_segmentation_server_amd.api import proto as P
    from semantic_segmentation_server_amd.api import service as S
    from semantic_segmentation_server_amd.runtime.engine import Engine
    from semantic_segmentation_server_amd.server import Server
    maps, seen = SC.speckled(33, 3, 65, 65, block=8)[0], []  # the model's output: speckled maps

    def infer(self, frames, bgr=None):
        m = maps[len(seen) % len(maps)][None].copy()
        seen.append(m.copy())
        return torch.from_numpy(m), None

    monkeypatch.setattr(Engine, "_infer", infer)
    srv = Server(_cfg(input_size=65, serve_masks=True, smooth_labels=1, fps_limit=None), max_steps=3).start()
    try:
        srv.producer.join(timeout=120)
        assert srv.producer.steps == 3 and srv.producer.error is None
        with grpc.insecure_channel(f"127.0.0.1:{srv.port}") as ch:
            m = S.SemanticSegmentationV2Stub(ch).GetSegmentationMask(P.MaskRequest(stream_id=0))
        eng = srv.engine
        assert eng.smooth_radius == 1 and (m.width, m.height) == (eng.crop_w, eng.crop_h)
        lab = MR.from_wire(m.run_labels, m.run_lengths, m.width, m.height)
        assert np.array_equal(lab, MR.decode(srv.hub.mask(0).words))
        # the served mask is the smoothed form of a map the model put out, and of no raw one
        cw, ch = eng.crop_w, eng.crop_h
        assert len(seen) >= 3 and not any(np.array_equal(lab, r[0, :ch, :cw]) for r in seen)
        assert any(np.array_equal(lab, SM.apply(r, None, cw, ch, 1)[0][0, :ch, :cw]) for r in seen)
    finally:
        srv.stop(0)


def test_step_all_on_the_cpu_smooths_before_every_host_encoder():
    from semantic_segmentation_server_amd.runtime.engine import Engine
    raw, _ = SC.speckled(32, 2, 129, 129, block=16)
    eng = Engine(_cfg(serve_masks=True, smooth_labels=2))
    eng.set_camera(160, 120)
    maps = iter(list(raw))
    eng._infer = lambda frames, bgr=None: (torch.from_numpy(next(maps).copy())[None], None)
    frames = torch.zeros((1, 120, 160, 3), dtype=torch.uint8)
    cw, ch = eng.crop_w, eng.crop_h
    sm, _ = SM.apply(raw, None, cw, ch, 2)
    for k in range(2):
        labels, _ = eng.run_device(frames)
        assert np.array_equal(labels[0].numpy(), sm[k])  # pad rows pass through
        assert np.array_equal(MR.decode(eng.mask_packed[0].numpy().view(np.uint32)), sm[k, :ch, :cw])
