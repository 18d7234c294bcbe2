"""The bf16 plan walker (tests/plan_bound.py) judged on the CPU.

Plans are built on ``torch.device("cpu")`` with the launches stubbed (planning only asks the
built extension for LDS sizes), filled with what a correct kernel of each picked family leaves
(``fill_from_emulation``: fp32 accumulation in two orders, roundings where the family's
reference has them) and walked with ``run=False``.

Positive: one representative pick of every family passes, in both accumulation orders. The
33-wide families (``stream*``, ``band*``) exist only in the 513 plan: there the block's input
buffer is filled with random bf16 values and that step alone is emulated and checked, which
teacher forcing permits. Negative: each injected fault is reported at exactly its buffer; the
steps after it are emulated from the damaged buffer, as a plan with one wrong kernel would run.
Structure: ``plan_steps`` matches the ops of every bf16 key of the tune file, through every
variant at every depth, launching nothing.
The reproducibility walk (``chip_poison``, the mode of the poisoned device ids): on a plan of
host ops (``emulated_ops``) a clean plan passes, an op that reads a hidden tensor the poison
callable NaN-fills is reported as P != A, one that adds its call count as not reproducible,
each at its buffer and variant.
"""
import json
import os
import sysconfig

import numpy as np
import pytest
import torch

import bound_cases as BC
import plan_bound as PB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TUNE = os.path.join(ROOT, "assets", "tune_mi355x.json")
_SO = os.path.join(ROOT, "semantic_segmentation_server_amd", "ops",
                   "_hip" + (sysconfig.get_config_var("EXT_SUFFIX") or ".so"))
pytestmark = pytest.mark.skipif(not os.path.exists(_SO), reason="extension not built (run build())")

_MODELS = {}


def _model(arch):
    from semantic_segmentation_server_amd.models.deeplab import build_model
    if arch not in _MODELS:
        _MODELS[arch] = build_model(arch, 21 if arch == "mnv2" else 19, calibrate_hw=65)
    return _MODELS[arch]


@pytest.fixture
def no_gpu(monkeypatch):
    """No launch, no tuning, no device call: what is left of plan building runs on the CPU."""
    from semantic_segmentation_server_amd.models.plan import HipPlanModel
    monkeypatch.setattr(HipPlanModel, "_launch", staticmethod(lambda ops, args: None))
    monkeypatch.setattr(HipPlanModel, "_autotune", lambda self, *a: setattr(self, "choices", {}))
    for name in ("SSA_TUNE_FILE", "SSA_RETUNE", "SSA_FUSED_IR", "SSA_GUARD_BYTES", "SSA_POOL_FORK",
                 "SSA_POOL_FUSED", "SSA_ROW_REPEAT"):
        monkeypatch.delenv(name, raising=False)


def _plan(arch, B, size, cw, ch):
    """(hm, ops, bufs, frames, lut_x, lut_y) of a fresh CPU plan on ``SyntheticSource`` frames."""
    from semantic_segmentation_server_amd import config as C
    from semantic_segmentation_server_amd.models.hip_model import HipDeepLab
    from semantic_segmentation_server_amd.ops import reference_ops as R
    from semantic_segmentation_server_amd.runtime.sources import SyntheticSource
    model = _model(arch)
    cfg = C.Config(arch=arch, dtype="bf16", input_size=size, batch=B, backend="hip", graph=False,
                   num_classes=model.num_classes)
    hm = HipDeepLab(model, torch.device("cpu"), cfg)
    ops, bufs = hm._plan(B, ch, cw)
    lx, ly, *_ = R.letterbox_luts(cw, ch, size, size)
    f, _, _ = SyntheticSource(cw, ch, pool=B, seed=13).read_batch(B)
    lut = lambda t: torch.tensor(np.array(t), dtype=torch.int32)  # noqa: E731
    return hm, ops, bufs, torch.from_numpy(np.array(f)), lut(lx), lut(ly)


def _set_picks(ops, want):
    """Pick, in every Choice at any depth, the first variant whose name starts with one of the
    prefixes ``want`` lists for that choice (``{choice name or kind: [prefix, ...]}``); the
    default elsewhere. Returns the (choice, variant) pairs that were set."""
    from semantic_segmentation_server_amd.models.plan import Choice
    done = []
    for op in ops:
        if not isinstance(op, Choice):
            continue
        for prefix in want.get(op.name, want.get(PB.choice_kind(op.name), ())):
            hit = next((i for i, (n, _) in enumerate(op.variants) if n.startswith(prefix)), None)
            if hit is not None:
                op.pick = hit
                done.append((op.name, op.variants[hit][0]))
                break
        for _, vops in op.variants:
            done += _set_picks(vops, want)
    return done


# one pick of every family that the 129 plans hold (the prefixes are tried in order)
MNV2_PICKS = [
    {"stem+block0": ["stem_band"], "block": ["slice", "dwpr", "dwproj"], "aspp.branches": ["grouped_v5+pool"],
     "aspp.head": ["head_g"]},
    {"stem+block0": ["stem_block0_"], "block": ["tile", "fused", "dwpw"], "aspp.branches": ["grouped_v17k2c"],
     "aspp.head": ["split"], "pw": ["pw"], "aspp.proj": ["v5"]},
    {"stem+block0": ["separate"], "block0": ["tile"], "block": ["fused", "dwproj", "unfused"], "pw": ["pw"],
     "aspp.branches": ["separate"], "rate": ["tapg"], "aspp.head": ["split"]},
    {"stem+block0": ["separate"], "block0": ["unfused"], "block": ["unfused"], "aspp.branches": ["separate"],
     "rate": ["v5g"], "aspp.head": ["head_g1w"]},
]


@pytest.mark.parametrize("order", ["whole", "parts"])
@pytest.mark.parametrize("picks", range(len(MNV2_PICKS)))
def test_emulated_mnv2_plan_passes(picks, order, no_gpu):
    hm, ops, bufs, frames, lx, ly = _plan("mnv2", 2, 129, 160, 120)
    done = dict(_set_picks(ops, MNV2_PICKS[picks]))
    assert set(MNV2_PICKS[picks]) <= {k for n in done for k in (n, PB.choice_kind(n))}, done
    PB.fill_from_emulation(hm, ops, bufs, frames, lx, ly, order=order)
    rep = PB.check_plan(hm, ops, bufs, frames, lx, ly, run=False)
    checked = {b for b, *_ in rep}
    assert {"b0_out", "b16_out", "aspp_cat", "img_bias", "logits", "labels"} <= checked, checked
    print(f"picks {picks} [{order}]: {len(rep)} checks, worst {PB.worst(rep)}")


@pytest.mark.parametrize("order", ["whole", "parts"])
@pytest.mark.parametrize("stem", ["fp32", "mfmaw16x32"])
def test_emulated_resnet_plan_passes(stem, order, no_gpu):
    hm, ops, bufs, frames, lx, ly = _plan("resnet50", 2, 129, 160, 120)
    assert dict(_set_picks(ops, {"stem": [stem]}))["stem"] == stem
    PB.fill_from_emulation(hm, ops, bufs, frames, lx, ly, order=order)
    rep = PB.check_plan(hm, ops, bufs, frames, lx, ly, run=False)
    checked = {b for b, *_ in rep}
    assert {"stem", "pool0", "r0_down", "r15_out", "aspp_cat", "img_bias", "logits", "labels"} <= checked, checked


@pytest.mark.parametrize("order", ["whole", "parts"])
@pytest.mark.parametrize("block,prefix", [(7, "stream8w"), (9, "stream32wh6c"), (13, "stream16h"), (14, "stream8L"),
                                          (16, "stream32Lh6"), (4, "band"), (5, "band2s1h")])
def test_emulated_wide_families_pass(block, prefix, order, no_gpu):
    """``stream*`` (raster, lattice, split hidden) and ``band*`` exist on the 513 plan's maps
    only: the block's input is random bf16 values, the block alone is emulated and checked."""
    hm, ops, bufs, frames, lx, ly = _plan("mnv2", 1, 513, 640, 480)
    name = f"block{block}"
    done = dict(_set_picks(ops, {name: [prefix]}))
    assert done[name].startswith(prefix)
    x = bufs[f"b{block - 1}_out"]
    x.copy_((torch.randn(x.shape, generator=torch.Generator().manual_seed(block)) * 0.7).to(x.dtype))
    PB.fill_from_emulation(hm, ops, bufs, frames, lx, ly, order=order, select=lambda n: n == name)
    rep = PB.check_plan(hm, ops, bufs, frames, lx, ly, run=False, select=lambda n: n == name)
    assert [(b, v) for b, v, *_ in rep] == [(f"b{block}_out", done[name])]


# ---------------------------------------------------------------- injected faults
def _two_ulps(buf):
    def fault(bufs):
        t = bufs[buf]
        at = np.unravel_index(int(t.float().abs().argmax()), tuple(t.shape))  # the largest ulp of the buffer
        before = float(t[at])
        t.view(torch.int16)[at] += 2  # the bf16 bit pattern stepped by exactly two (away from zero)
        assert abs(float(t[at]) - before) == 2 * 2.0 ** (np.floor(np.log2(abs(before))) - 7), (before, float(t[at]))
    return fault


def _group_from_next_row(bufs):
    t = bufs["b3_out"]  # 17 x 17 x 32: columns 0 .. 15 of row 5 of image 1 from row 6
    t[1, 5, :16] = t[1, 6, :16].clone()


def _branch_shifted(bufs):
    t = bufs["aspp_cat"]  # the rate-6 branch (co_off 256) written at co_off + 8
    t[..., 264:520] = t[..., 256:512].clone()


def _constant_row_from_a_live_row(bufs):
    t = bufs["b0_out"]  # 65 rows, camera rows end at input row 97: output rows 50 .. 64 are constant
    assert torch.equal(t[:, 55], t[:, 56]) and not torch.equal(t[:, 55], t[:, 30])
    t[:, 55] = t[:, 30].clone()


def _pad_channel(bufs):
    bufs["logits"][1, 3, 4, 22] = 0.5


SIMPLE_FAULTS = {  # id -> (step after which the buffer is damaged, buffer, damage, picks)
    "two-ulps-block-out": ("block5", "b5_out", _two_ulps("b5_out"), 0),
    "column-group-from-next-row": ("block3", "b3_out", _group_from_next_row, 0),
    "branch-at-co_off+8": ("aspp.branches", "aspp_cat", _branch_shifted, 0),
    "constant-row-from-live-row": ("stem+block0", "b0_out", _constant_row_from_a_live_row, 0),
    "pad-channel-written": ("aspp.head", "logits", _pad_channel, 0),
}


def _reported(hm, ops, bufs, frames, lx, ly):
    with pytest.raises(PB.PlanCheckError) as err:
        PB.check_plan(hm, ops, bufs, frames, lx, ly, run=False)
    print(err.value)
    return {b for b, _, _ in err.value.failures}


@pytest.mark.parametrize("case", sorted(SIMPLE_FAULTS))
def test_fault_is_reported_at_its_buffer(case, no_gpu):
    after, buf, damage, picks = SIMPLE_FAULTS[case]
    hm, ops, bufs, frames, lx, ly = _plan("mnv2", 2, 129, 160, 120)
    _set_picks(ops, MNV2_PICKS[picks])
    hit = []

    def fault(step, bufs_, redo):
        if step == after:
            damage(bufs_)
            hit.append(step)
    PB.fill_from_emulation(hm, ops, bufs, frames, lx, ly, fault=fault)
    assert hit == [after]
    assert _reported(hm, ops, bufs, frames, lx, ly) == {buf}


def test_fault_dropped_tap_of_the_rate12_branch(no_gpu):
    """On the 9 x 9 map of the 129 plan the centre tap is the rate-12 branch's only live one
    (12 > 8): the branch is written without it (``sum_taps(skip=(1, 1))``: bias only)."""
    hm, ops, bufs, frames, lx, ly = _plan("mnv2", 2, 129, 160, 120)
    _set_picks(ops, MNV2_PICKS[0])
    (w, b), rate = PB._dense(hm.aspp_atrous[1][0]), hm.aspp_atrous[1][1]
    assert rate == 12

    def fault(step, bufs_, redo):
        if step == "aspp.branches":
            x = bufs_["b16_out"].permute(0, 3, 1, 2).float()
            acc = BC.sum_taps(x, w.float(), 1, rate, skip=(1, 1)) + b[None, :, None, None]
            bufs_["aspp_cat"][..., 512:768] = torch.relu(acc).permute(0, 2, 3, 1).to(torch.bfloat16)
    PB.fill_from_emulation(hm, ops, bufs, frames, lx, ly, fault=fault)
    assert _reported(hm, ops, bufs, frames, lx, ly) == {"aspp_cat"}


@pytest.mark.parametrize("picks,buf", [(0, "logits"), (1, "aspp_proj")])
def test_fault_image0_bias_used_for_image1(picks, buf, no_gpu):
    """The head is emulated again from a bias buffer whose row 1 holds image 0's bias (the fused
    head: the logits; the split head: the projection, and the logits that follow from it)."""
    hm, ops, bufs, frames, lx, ly = _plan("mnv2", 2, 129, 160, 120)
    _set_picks(ops, MNV2_PICKS[picks])

    def fault(step, bufs_, redo):
        if step == "aspp.head":
            keep = bufs_["img_bias"].clone()
            bufs_["img_bias"][1] = keep[0]
            redo()
            bufs_["img_bias"].copy_(keep)
    PB.fill_from_emulation(hm, ops, bufs, frames, lx, ly, fault=fault)
    assert _reported(hm, ops, bufs, frames, lx, ly) == {buf}


def test_fault_projection_residual_omitted(no_gpu):
    hm, ops, bufs, frames, lx, ly = _plan("mnv2", 2, 129, 160, 120)
    _set_picks(ops, MNV2_PICKS[0])
    assert hm.blocks[8]["spec"].residual

    def fault(step, bufs_, redo):
        if step == "block8":
            bufs_["b8_out"].copy_((bufs_["b8_out"].float() - bufs_["b7_out"].float()).to(torch.bfloat16))
    PB.fill_from_emulation(hm, ops, bufs, frames, lx, ly, fault=fault)
    assert _reported(hm, ops, bufs, frames, lx, ly) == {"b8_out"}


# ---------------------------------------------------------------- the reproducibility walk
def _poisoned_walk(wrong, steps=("block5", "block8", "upsample")):
    """``check_plan(chip_poison=...)`` over ``steps`` of an emulated plan with host ops
    (``plan_bound.emulated_ops``), the picks only; ``wrong(step, call, bufs, hidden, calls)``
    wraps the last leaf call of each step's pick. The poison callable NaN-fills ``hidden``, the
    stand-in for on-chip state. Returns (picks by step, report)."""
    hm, ops, bufs, frames, lx, ly = _plan("mnv2", 2, 129, 160, 120)
    _set_picks(ops, MNV2_PICKS[0])
    PB.fill_from_emulation(hm, ops, bufs, frames, lx, ly)
    hops = PB.emulated_ops(hm, ops, bufs, frames, lx, ly)
    hidden, calls, picks = torch.zeros(1), [0], {}
    for op in hops:
        if getattr(op, "name", None) in steps:
            vname, leaves = op.variants[op.pick]
            picks[op.name] = vname
            leaves[-1] = wrong(op.name, leaves[-1], bufs, hidden, calls)
    assert set(picks) == set(steps)
    # the unselected steps are only executed: no-ops here, their buffers are filled already
    hops = [op if getattr(op, "name", None) in steps else type(op)(op.name, [("op", [])]) if hasattr(op, "variants")
            else (lambda *a: None) for op in hops]
    wk = PB.Walker(hm, hops, bufs, frames, lx, ly, run=True, every_variant=False, select=lambda n: n in steps,
                   chip_poison=lambda: hidden.fill_(float("nan")), upsample_fields=False)
    return picks, wk


def test_poisoned_walk_passes_on_clean_ops(no_gpu):
    picks, wk = _poisoned_walk(lambda step, call, bufs, hidden, calls: call)
    rep = wk.walk()
    # one entry per leaf call, named by the first buffer it writes (block 8's pick has two)
    assert {("b5_out", picks["block5"]), ("b8_out", picks["block8"]), ("labels", f"plan/{picks['upsample']}")} <= \
        {(b, v) for b, v, *_ in rep}
    assert wk.leaves == len(rep) >= 3


def test_poisoned_walk_sees_stale_state_and_a_call_counter(no_gpu):
    """An op that adds a hidden host tensor (NaN once poisoned, cleared by the op as a kernel
    overwrites its LDS) is reported as P != A at its buffer and variant; one that adds its call
    count as not reproducible; the clean steps beside them are not reported."""
    def wrong(step, call, bufs, hidden, calls):
        def stale(*a):
            call(*a)
            t = bufs["b5_out"]
            t[1, 2, 3, 4] = t[1, 2, 3, 4].float() + hidden[0]
            hidden.zero_()  # the kernel leaves its own bytes behind

        def counter(*a):
            call(*a)
            calls[0] += 1
            bufs["b8_out"][0, 1, 0, 2] = float(calls[0])
        return {"block5": stale, "block8": counter}.get(step, call)
    picks, wk = _poisoned_walk(wrong)
    with pytest.raises(PB.PlanCheckError) as err:
        wk.walk()
    print(err.value)
    fails = err.value.failures
    p5 = [m for b, v, m in fails if (b, v) == ("b5_out", picks["block5"])]
    assert len(p5) == 1 and "the poisoned run differs: P != A at 1 of" in p5[0] and p5[0].endswith("first at (1, 2, 3, 4)")
    p8 = [m for b, v, m in fails if (b, v) == ("b8_out", picks["block8"])]
    assert p8 and "not reproducible: A' != A at 1 of" in p8[0] and p8[0].endswith("first at (0, 1, 0, 2)")
    assert {b for b, _, _ in fails} == {"b5_out", "b8_out"}


def test_variant_without_a_family_is_an_error(no_gpu):
    hm, ops, bufs, frames, lx, ly = _plan("mnv2", 2, 129, 160, 120)
    blk = next(op for op in ops if getattr(op, "name", "") == "block7")
    blk.variants.append(("resident4", blk.variants[0][1]))
    with pytest.raises(AssertionError, match="block7/resident4: a variant without a reference family"):
        PB.Walker(hm, ops, bufs, frames, lx, ly, run=False).structure()


def test_upsample_fields_are_decided():
    """The ``make_logits`` fields the device test writes into the logits buffer leave at most
    MAX_UNDECIDED of the map under the margin, at both plan geometries (on the CPU, float64)."""
    import upsample_ref as UR
    for B, h, H in ((3, 9, 129), (2, 33, 513)):
        for field, seed in PB.UPSAMPLE_FIELDS:
            lg = UR.make_logits(B, h, h, 21, 24, field, seed)
            arg, ok, scale = PB.label_ref(lg, 21, H, H)
            assert 1.0 - ok.double().mean().item() <= UR.MAX_UNDECIDED, (h, field)
            assert arg.unique().numel() >= 8, (h, field, arg.unique())


@pytest.mark.parametrize("key", sorted(k for k in json.load(open(TUNE)) if "int8" not in k.split(":")[0]))
def test_plan_steps_match_the_ops(key, no_gpu):
    """Every bf16 key of the tune file (the int8 plan has its own walker, tests/int8_ref.py):
    the step list matches the ops, and every variant at every depth has a family, as many
    described ops as it has ops and its nested choices where they are expected."""
    from semantic_segmentation_server_amd import config as C
    from semantic_segmentation_server_amd.models.hip_model import HipDeepLab
    kind, b, cam, size = key.split(":")
    B, S = int(b[2:]), int(size[3:])
    Wc, Hc = (int(v) for v in cam[len("cam="):].split("x"))
    model = _model(kind)
    hm = HipDeepLab(model, torch.device("cpu"), C.Config(
        arch=kind, dtype="bf16", input_size=S, batch=B, backend="hip", graph=False, num_classes=model.num_classes))
    ops, bufs = hm._plan(B, Hc, Wc)
    frames = torch.zeros(B, Hc, Wc, 3, dtype=torch.uint8)
    from semantic_segmentation_server_amd.ops import reference_ops as R
    lx, ly, *_ = R.letterbox_luts(Wc, Hc, S, S)
    seen = PB.Walker(hm, ops, bufs, frames, np.array(lx), np.array(ly), run=False).structure()
    saved = json.load(open(TUNE))[key]
    assert seen >= len(saved)
    print(f"{key}: {len(ops)} ops, {seen} variants")
