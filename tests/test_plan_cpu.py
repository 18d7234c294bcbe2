"""The plan structure as a contract, checked on the CPU (models/plan.py).

``assets/tune_mi355x.json`` addresses plan steps and their variants by name, and a saved name
that no longer exists is silently re-timed at start-up, which changes the kernels that run
and the rounding of the output. Plans are built on ``torch.device("cpu")`` with the launches
stubbed: planning only asks the built extension for LDS sizes."""
import json
import os
import sysconfig

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TUNE = os.path.join(ROOT, "assets", "tune_mi355x.json")
_SO = os.path.join(ROOT, "semantic_segmentation_server_amd", "ops",
                   "_hip" + (sysconfig.get_config_var("EXT_SUFFIX") or ".so"))
pytestmark = pytest.mark.skipif(not os.path.exists(_SO), reason="extension not built (run build())")

_MODELS = {}


def _hip_model(kind, B, size):
    """A HIP model of the tune file's ``kind`` on the CPU (classes as in BASELINE.json)."""
    from semantic_segmentation_server_amd import config as C
    from semantic_segmentation_server_amd.models import quant
    from semantic_segmentation_server_amd.models.deeplab import build_model, synthetic_normalized
    from semantic_segmentation_server_amd.models.hip_int8 import HipDeepLabInt8
    from semantic_segmentation_server_amd.models.hip_model import HipDeepLab
    arch, ncls = ("mnv2", 21) if kind == "mnv2" else ("resnet50", 19)
    if arch not in _MODELS:
        model = build_model(arch, ncls, calibrate_hw=65)
        scales = None
        if arch == "resnet50":
            x = synthetic_normalized(2, 65, 65, torch.Generator().manual_seed(11))
            scales = quant.calibrate(model.float(), x)
        _MODELS[arch] = model, scales
    model, scales = _MODELS[arch]
    cfg = C.Config(arch=arch, dtype="int8" if kind.endswith("int8") else "bf16", input_size=size,
                   batch=B, backend="hip", graph=False, num_classes=ncls)
    if kind.endswith("int8"):
        return HipDeepLabInt8(model, torch.device("cpu"), cfg, scales=scales)
    return HipDeepLab(model, torch.device("cpu"), cfg)


@pytest.fixture
def no_gpu(monkeypatch):
    """No launch, no device call: what is left of plan building and tuning runs on the CPU."""
    from semantic_segmentation_server_amd.models.plan import HipPlanModel
    monkeypatch.setattr(HipPlanModel, "_launch", staticmethod(lambda ops, args: None))
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a: None)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
    for name in ("SSA_TUNE_FILE", "SSA_RETUNE", "SSA_RETUNE_ONLY", "SSA_LOG_AUTOTUNE", "RANK",
                 "SSA_FUSED_IR", "SSA_GUARD_BYTES", "SSA_POOL_FORK"):
        monkeypatch.delenv(name, raising=False)


@pytest.fixture
def no_tune(no_gpu, monkeypatch):
    from semantic_segmentation_server_amd.models.plan import HipPlanModel
    monkeypatch.setattr(HipPlanModel, "_autotune", lambda self, *a: setattr(self, "choices", {}))


def _walk(ops):
    """Every Choice of a plan, at any depth, in order."""
    from semantic_segmentation_server_amd.models.plan import Choice
    for op in ops:
        if isinstance(op, Choice):
            yield op
            for _, vops in op.variants:
                yield from _walk(vops)


def _structure(ops):
    from semantic_segmentation_server_amd.models.plan import Choice
    return [[op.name, [[n, _structure(v)] for n, v in op.variants]] if isinstance(op, Choice) else None
            for op in ops]


@pytest.mark.parametrize("key", sorted(json.load(open(TUNE))))
def test_committed_picks_resolve(key, no_tune):
    """Every step the tune file names is a Choice of the plan of that shape, its saved variant
    is one of that choice's variants, and the plan has no choice the file does not know."""
    from semantic_segmentation_server_amd.models.plan import all_choices
    saved = json.load(open(TUNE))[key]
    kind, b, cam, size = key.split(":")
    Wc, Hc = (int(v) for v in cam[len("cam="):].split("x"))
    hm = _hip_model(kind, int(b[2:]), int(size[3:]))
    assert hm.kind == kind
    ops, _ = hm._plan(int(b[2:]), Hc, Wc)
    variants = {c.name: [n for n, _ in c.variants] for c in all_choices(ops)}
    # (a choice shared by two variants of its parent, block{i}.expand, is listed once per variant)
    assert len(variants) == len({id(c) for c in all_choices(ops)}), "two choices share a name"
    assert {id(c) for c in _walk(ops)} == {id(c) for c in all_choices(ops)}, "choices nest deeper"
    unresolved = {n: v for n, v in saved.items() if v not in variants.get(n, ())}
    assert not unresolved, f"{key}: saved picks that the plan does not have: {unresolved}"
    assert sorted(variants) == sorted(saved), f"{key}: choices missing from the tune file"


@pytest.mark.parametrize("kind,B", [("mnv2", 2), ("resnet50_int8", 1)])
def test_plan_copies_are_identical_and_take_the_picks(kind, B, no_tune):
    from semantic_segmentation_server_amd.models.plan import all_choices, copy_picks
    hm = _hip_model(kind, B, 129)
    (ops0, bufs0), (ops1, bufs1) = hm._plan(B, 120, 160), hm._plan(B, 120, 160, part=1)
    assert set(hm._plans) == {(B, 120, 160), (B, 120, 160, 1)}
    assert ops0 is not ops1 and _structure(ops0) == _structure(ops1)
    desc = [[(n, tuple(t.shape), t.dtype) for n, t in b.items()] for b in (bufs0, bufs1)]
    assert desc[0] == desc[1]
    assert all(bufs0[n].data_ptr() != bufs1[n].data_ptr() for n in ("stem", "logits", "labels"))
    every = all_choices(ops0)
    nested = [c for c in every if c not in ops0 and len(c.variants) > 2]
    moved = [next(c for c in ops0 if c in every and len(c.variants) > 2), (nested or every)[-1]]
    assert moved[0] is not moved[1]
    moved[0].pick, moved[1].pick = 2, 1
    copy_picks(ops0, ops1)
    picks = [[c.pick for c in _walk(ops)] for ops in (ops0, ops1)]
    assert picks[0] == picks[1] and sorted(picks[1])[-2:] == [1, 2]
    if kind == "resnet50_int8":
        for ops in (ops0, ops1):
            names = [c.name for c in _walk(ops) if c.name.startswith("i8conv")]
            assert names == [f"i8conv{k}" for k in range(1, 16 * 3 + 4 + 2 + 1)]
    else:
        assert nested, "the mnv2 plan nests choices (block{i}.expand, aspp.b0, ...)"


def test_tune_file_round_trip(no_gpu, monkeypatch, tmp_path):
    """A cold tune times every top-level choice and writes its key; a model that reads the file
    times nothing; an unknown saved variant, or SSA_RETUNE_ONLY, re-times exactly that choice."""
    from semantic_segmentation_server_amd.models.plan import Choice, all_choices
    timed = []

    def autotune(self, args, reps=5):
        timed.append(self.name)
        self.pick = 1 if len(self.variants) > 1 else 0
    monkeypatch.setattr(Choice, "autotune", autotune)
    path = tmp_path / "tune.json"
    monkeypatch.setenv("SSA_TUNE_FILE", str(path))
    key = "mnv2:B=1:cam=160x120:in=129"

    def build():
        timed.clear()
        hm = _hip_model("mnv2", 1, 129)
        return hm, hm._plan(1, 120, 160)[0]

    hm, ops = build()
    top = [op.name for op in ops if isinstance(op, Choice)]
    assert timed == top and all(len(op.variants) > 1 for op in ops if isinstance(op, Choice))
    first = dict(hm.choices)
    assert first == {c.name: c.variants[c.pick][0] for c in all_choices(ops)} and len(first) > len(top)
    assert all(c.pick == (1 if c.name in top else 0) for c in all_choices(ops))
    assert json.load(open(path)) == {key: first}

    before = os.stat(path).st_mtime_ns
    hm, ops = build()  # picks from the file: nothing is timed, nothing is written
    assert timed == [] and hm.choices == first and os.stat(path).st_mtime_ns == before

    nested = next(n for n in first if n not in top)
    path.write_text(json.dumps({key: dict(first, upsample="no_such_variant", **{nested: "gone"})}))
    hm, ops = build()  # an unknown variant of a nested choice keeps its default, untimed
    assert timed == ["upsample"] and hm.choices == first
    assert json.load(open(path)) == {key: first}

    monkeypatch.setenv("SSA_RETUNE_ONLY", "block3")
    block3 = next(c for c in ops if getattr(c, "name", "") == "block3")
    path.write_text(json.dumps({key: dict(first, block3=block3.variants[0][0])}))
    hm, ops = build()
    assert timed == ["block3"] and hm.choices == first
    assert json.load(open(path)) == {key: first}
    assert os.listdir(tmp_path) == ["tune.json"]  # the atomic replace left no temporary
