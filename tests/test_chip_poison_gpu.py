"""The control of tests/chip_poison.py, and the served kernels outside the plans on poisoned
LDS and registers.

Control: after ``poison()`` every word the LDS probe and the register probe read, on every
workgroup, is the pattern, and the probes ran on every CU / SIMD of the device. Without a
preceding poison the same figures are printed only.

Served kernels: each case is the smallest adversarial case of the kernel's own module, run
through that module's own harness (imported, not copied), eager, three times: A, A' and P. In P
every launch of the listed ``hip_ops`` entry points is preceded by ``poison()`` on the same
stream; a wrapper with several kernels (``class_regions``: seven, ``postprocess``: its chain) is
poisoned before its first. The harness asserts its integer definition (or, for the fp32 pools
and the confidence codes, its float64 bound) in all three runs, P included, and the words every
call left in its outputs and in its carried state are bit-equal between A, A' and P.
The carried state of the stateful chains (track ids, dwell, event state, stable labels) is
compared after every call, so a state that does not survive a poisoned call fails there.
Captured graphs are out of scope: a poison launch cannot be interleaved into a replay.

Words read as an index or address from LDS, checked in the kernels' code to be written by the
kernel itself before they are read (a poisoned one would be a wild pointer, not a wrong value):
  postprocess.hip: k_ccl_local lbl / fgrow / bgrow / s_nroot (all of the tile, tid 0, before the
    first barrier); k_ccl_merge par / minr / rp / toff / part / s_c (rp: every i < R by the tile
    lists or the rovf list, which is complete whenever R <= kMergeCap); the accumulation tables'
    keys (zeroed before the first barrier) and anc / nanc / deep (every slot); assign_frame s_key
    (k < total, padding to n2), s_cnt, s_w; finalize_frame s_sn (i < kept), s_order (a
    permutation of [0, ns)), s_deep; k_records s_res.
  class_regions.hip: lab / par / size and slot / acc (every tile pixel), key (i < n2), hkey / hcnt
    (all kHash), p_lab / p_pix (tid < n_prev, read for j < n_prev), best / wkey (every tid),
    p_id / p_age / wave_new (every thread, every wave, both halves before they are read).
  zone_events.hip: cur_id (tid < cn, read for k < cn), succ (tid < pn, read for b < pn; it indexes
    the current row), wave_total (every wave). zone_presence.hip / zone_stats.hip: tab (zeroed over
    the used words). mask_rle.hip: red / wtot (every wave). label_stable.hip, yuv422.hip: no LDS.
  model_ops.hip (pools, matvec, upsample_argmax_conf): LDS holds values only.
The plans' kernels (tests/test_bf16_plan.py, tests/test_int8_plan.py poisoned ids):
  fused_ir_stream.hip s_opix (i < p1 - p0, read for px < p1 - p0) and s_flag (tid 0, between two
    barriers); stem_band.hip sly (i < n_rows, read at min(rel_row, n_rows - 1)); conv_gemm.hip /
    tap_conv.hip / conv_i8.hip s_tap / s_tapmask (zeroed by tid 0 before the barrier, then ORed)
    and s_flag; the span, lattice, permutation and tile-order tables are read from global memory,
    never staged in LDS; LDS-DMA row addresses are per-lane registers computed from them.
"""
import contextlib
import inspect

import numpy as np
import pytest
import torch

import chip_poison as CP

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------- the control
def test_poison_reaches_every_lds_word_and_probed_register():
    covers = (("LDS", CP.lds_coverage), ("registers", CP.reg_coverage))
    for name, cover in covers:  # informative: what the kernels before this test left behind
        bad, n, units, want = cover(False)
        print(f"{name} probe without a poison: {n - bad} of {n} words hold the pattern; ran on {units} of {want} units")
    for name, cover in covers:
        bad, n, units, want = cover(True)
        print(f"{name} probe after poison(): {n - bad} of {n} words hold the pattern; ran on {units} of {want} units")
        assert units == want, f"the {name} probe ran on {units} of {want} units: raise the block counts"
        assert bad == 0, f"{name}: {bad} of {n} probed words are not the pattern after poison()"


# ---------------------------------------------------------------- A / A' / P of the served kernels
# hip_ops entry point -> the arguments it writes that a caller reads: outputs and carried state
# (workspaces hold atomics' arrival order and are no output)
WRITES = {
    "postprocess": (),  # its record rows are defined up to 1 + 5 n words: compared by the case
    "mask_rle": ("out",), "mask_rle_copy_to_host": ("dst",),
    "class_regions": ("out",), "region_tracks": ("out", "state"), "zone_stats": ("out",),
    "zone_presence": ("out", "state"), "zone_events": ("out", "state"),
    "label_stable": ("labels_out", "conf_out", "state"),
    "upsample_argmax_conf": ("labels", "conf"), "yuv422_to_bgr": ("out",),
    "aspp_pool": ("img_bias",), "global_avgpool": ("out",), "matvec": ("out",),
    "global_avgpool_i8": ("out",), "maxpool3x3s2_i8": ("out",), "maxpool3x3s2": ("out",),
}


@contextlib.contextmanager
def _recording(names, poisoned):
    """Every call of ``hip_ops.<name>`` (preceded by ``poison()`` if ``poisoned``) is followed by
    a sync and a copy of what it wrote -> [(entry point, argument, tensor)]."""
    from semantic_segmentation_server_amd.ops import hip_ops
    log = []
    with pytest.MonkeyPatch.context() as mp:
        for name in names:
            orig = getattr(hip_ops, name)
            sig = inspect.signature(orig)

            def wrapped(*a, _orig=orig, _sig=sig, _name=name, **kw):
                if poisoned:
                    CP.poison()
                ret = _orig(*a, **kw)
                torch.cuda.synchronize()
                bound = _sig.bind(*a, **kw).arguments
                log.append((_name, "", None))
                for arg in WRITES[_name]:
                    t = bound.get(arg)
                    if torch.is_tensor(t):
                        log.append((_name, arg, t.detach().clone()))
                return ret
            mp.setattr(hip_ops, name, wrapped)
        yield log


def _three(case, names, least=1):
    """``case()`` (which asserts its own definition, and may return further tensors to compare)
    as A, A' and P. ``least``: the launches that must have been poisoned."""
    CP.require()
    runs = []
    try:
        for tag in ("A", "A'", "P"):
            with _recording(names, tag == "P") as log:
                extra = case() or []
            tensors = [(f"{n}.{a}#{i}", t) for i, (n, a, t) in enumerate(log) if t is not None]
            tensors += [(f"result#{i}", t if torch.is_tensor(t) else torch.from_numpy(np.ascontiguousarray(t).view(
                {1: np.uint8, 2: np.int16, 4: np.int32, 8: np.int64}[t.dtype.itemsize]))) for i, t in enumerate(extra)]
            runs.append((sum(t is None for _, _, t in log), tensors))
    except AssertionError:
        raise
    except RuntimeError as err:  # a device fault: nothing more is launched on this GPU
        pytest.exit(f"{case}: {err}", returncode=3)
    calls, a = runs[0]
    assert calls >= least and len(a) > 0, (calls, len(a))
    bad = []
    for what, (n, other) in (("not reproducible: A' != A", runs[1]), ("the poisoned run differs: P != A", runs[2])):
        assert n == calls and [k for k, _ in other] == [k for k, _ in a], (what, n, calls)
        bad += CP.same_bits([t for _, t in other], [t for _, t in a], [k for k, _ in a], what)
    assert not bad, f"{len(bad)} outputs differ:\n" + "\n".join(bad)
    print(f"{calls} launches poisoned, {len(a)} outputs: A = A' = P")


# accum mode -> a case of tests/post_cases.py: the union-find fallback, a crowded frame on the
# compact merge (rovf list), the full LDS tables of the accumulation kernels
POST = {1: "fallback_small-area4", 2: "rovf_compact-area4", 0: "tables_full"}


@pytest.mark.parametrize("accum", sorted(POST))
def test_postprocess(accum, monkeypatch):
    import post_cases as PC
    import test_postprocess_topology_gpu as TP
    monkeypatch.setenv("SSA_POST_ACCUM", str(accum))
    case = PC.BY_NAME[POST[accum]]
    _three(lambda: TP._defined(TP._check_case(case, PC.MIXED)), ["postprocess"])


def test_mask_rle_and_its_copy():
    import test_mask_rle_gpu as TM

    def case():
        TM.test_chunk_boundary("straddle")
        TM.test_copy_to_host_moves_only_the_used_words()
    _three(case, ["mask_rle", "mask_rle_copy_to_host"], least=2)


@pytest.mark.parametrize("with_conf", [False, True], ids=["6w", "7w"])
def test_class_regions(with_conf):
    import region_cases as RC
    import test_regions_paths_gpu as TR
    pos = sorted(RC.WIN_POS)[0]
    labels, conf = RC.window_batch(pos, RC.WIN_BATCHES - 1)
    want = RC.window_want(pos, RC.WIN_BATCHES - 1, with_conf)

    def case():
        bufs = TR.Buffers.for_call(labels.shape[0], TR.WIN_GEOMETRY["crop_h"], TR.WIN_GEOMETRY["crop_w"],
                                   TR.WIN_GEOMETRY["K"], with_conf)
        return [TR.run_and_compare(bufs, labels, conf if with_conf else None, want, **TR.WIN_GEOMETRY)]
    _three(case, ["class_regions"])


def test_full_chain_two_streams_three_calls():
    """class_regions, region_tracks, zone_presence and zone_events of ``test_events_gpu._Full`` on
    two streams (two rows and one a call), poisoned before every one of them in every call; the
    event words equal the CPU definition's and the carried states are compared after every call."""
    import presence_cases as PC
    import test_events_gpu as TE

    def case():
        s0, s1 = (list(s) for s in PC.sequences())
        w0, w1 = TE._seq_wants()
        full = TE._Full([2, 1])
        got0, got1 = [], []
        for k in range(3):
            ev = full.step(s0[2 * k:2 * k + 2] + s1[k:k + 1])
            got0 += [ev[0].copy(), ev[1].copy()]
            got1.append(ev[2].copy())
        TE._same(got0, w0[:6])
        TE._same(got1, w1[:3])
        return got0 + got1 + [full.chain.state, full.chain.pstate, full.ev.state]
    _three(case, ["class_regions", "region_tracks", "zone_presence", "zone_events"], least=12)


def test_label_stable_and_zone_stats():
    import test_stable_gpu as TS
    import test_zones_gpu as TZ

    def case():
        TS.test_batch_layouts_over_three_calls([3, 0, 2])
        TZ.test_three_frames_of_three_kinds_share_one_plane()
        TZ.test_confidence_blocks("random")
    _three(case, ["label_stable", "zone_stats"], least=5)


def test_upsample_argmax_conf():
    import test_confidence_gpu as TC
    _three(lambda: TC.test_kernel_against_float64(*TC.CASES[0], "noise"), ["upsample_argmax_conf"])


def test_yuv422_to_bgr():
    import test_raw_ingest_gpu as TY
    _three(TY.test_vector_body_and_tail_in_every_alignment_phase, ["yuv422_to_bgr"], least=18)


def test_pools_and_matvec():
    """``aspp_pool``, ``global_avgpool`` + ``matvec`` (with the bf16 max pool of the same test),
    ``global_avgpool_i8`` and ``maxpool3x3s2_i8`` at the smallest shapes of their own tests."""
    import bound_cases as BC
    import test_hip_kernels as TK

    def case():
        TK.test_aspp_pool(*BC.ASPP_POOL[-1])
        TK.test_maxpool_gap_matvec()
        TK.test_matvec(*BC.MATVEC[-1])
        TK.test_global_avgpool_i8(2, 50, 40)
        TK.test_global_avgpool_i8(3, 37, 528)
        TK.test_maxpool_i8(1, 7, 32)
    _three(case, ["aspp_pool", "global_avgpool", "matvec", "global_avgpool_i8", "maxpool3x3s2_i8", "maxpool3x3s2"],
           least=8)
