"""CPU tier of the int8 checks: the oracle (models/quant.py) that every GPU int8 test is
measured against, and the comparator those tests use, are pinned here without a GPU."""
import pytest
import torch
import torch.nn.functional as F

import int8_ref as I
from semantic_segmentation_server_amd.models import quant
from semantic_segmentation_server_amd.models.layers import ConvBNAct, init_random


def _layer(cin, cout, k, stride=1, dil=1, act=None, seed=0):
    layer = ConvBNAct(cin, cout, k, stride, dil, act=act)
    init_random(layer, seed)
    with torch.no_grad():  # a folded BN that is not the identity
        g = torch.Generator().manual_seed(seed + 1)
        layer.bn.running_mean.copy_(0.2 * torch.randn(cout, generator=g))
        layer.bn.running_var.copy_(0.5 + torch.rand(cout, generator=g))
    return layer.eval()


@pytest.mark.parametrize("act", [None, "relu"])
@pytest.mark.parametrize("res", [False, True])
@pytest.mark.parametrize("dil", [1, 6])
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("k", [1, 3])
def test_int8_conv_codes_is_exact(k, stride, dil, res, act):
    """``int8_conv_codes`` (fp32 convs over 576-term chunks summed in float64) against ONE
    direct float64 conv of the same codes and ``_qw`` weights with the float64 epilogue
    acc * s_in * s_w + b (+ res * s_res), ReLU, round-half-even, clamp +-127: bit-equal.
    Cin = 2048 makes 4 (1x1) / 32 (3x3) chunks."""
    B, H, Cin, Cout = 2, 9, 2048, 32
    layer = _layer(Cin, Cout, k, stride, dil, act=act, seed=3 + k)
    g = torch.Generator().manual_seed(17)
    x = torch.randint(-127, 128, (B, Cin, H, H), generator=g, dtype=torch.int32)
    wq, sw, b = quant._qw(layer)
    assert wq.abs().max() == 127 and bool((wq == wq.round()).all())
    OH = (H - 1) // stride + 1
    r = torch.randint(-127, 128, (B, Cout, OH, OH), generator=g, dtype=torch.int32) if res else None
    s_in, s_res = 0.02, 0.03
    v = I.exact_conv(x, wq, sw, b, s_in, stride=stride, dil=dil, res_codes=r, s_res=s_res, act=act)
    s_out = float(torch.quantile(v.abs().flatten(), 0.99)) / 127.0  # the largest 1 % clamp
    ref = I.requant(v, s_out)
    assert 0 < I.saturated_share(ref) < 0.05 and ref.unique().numel() > 50
    got = quant.int8_conv_codes(layer, x.float(), s_in, s_out, None if r is None else r.float(), s_res,
                                act=act)
    assert got.dtype == torch.int32 and torch.equal(got, ref)


def test_fake_quant_forward_is_the_chain_of_int8_conv_codes(monkeypatch):
    """``fake_quant_forward`` (the fp32 replay the GPU tests bound the logits with) against
    the chain stem codes -> F.max_pool2d -> blocks -> ASPP -> projection of exact
    ``int8_conv_codes`` calls, on a ResNet-50 at 65^2, B = 1. Every quantisation point of
    the replay is recorded (``quant.q``) and every link of the chain starts from the
    replay's own codes of the layer before (teacher forcing, as everywhere in these tests:
    the random-init network amplifies one flipped tie from block to block, which says
    nothing about either side). After dequantisation a layer may differ by one step on at
    most 1e-3 of its codes: fp32 and float64 differ only at rounding ties."""
    from semantic_segmentation_server_amd.models.deeplab import build_model, synthetic_normalized
    model = build_model("resnet50", 19, calibrate_hw=65).float().eval()
    x = synthetic_normalized(1, 65, 65, torch.Generator().manual_seed(5))
    S = quant.calibrate(model, x)
    rec = []
    real_q = quant.q

    def q_rec(t, s):
        out = real_q(t, s)
        rec.append((out, s))
        return out

    monkeypatch.setattr(quant, "q", q_rec)
    logits = quant.fake_quant_forward(model, S, x)
    monkeypatch.undo()
    it = iter(rec)

    def close(codes, s, what):
        out, s_rec = next(it)
        assert s_rec == s, what
        # compared after dequantisation, in steps; the replay's fp32 product code * s is
        # within 127 * 2^-24 steps of the exact one
        d = ((codes.double() * s - out.double()) / s).abs()
        assert float(d.max()) <= 1.0 + 127 * 2.0 ** -23 and (d > 0.5).double().mean().item() <= 1e-3, \
            (what, float(d.max()), (d > 0.5).double().mean().item())
        return torch.round(out / s)  # the replay's own codes feed the next link

    bb, a = model.backbone, model.aspp
    h = close(I.stem_ref_codes(x, bb.stem, S["stem"], bf16_operands=False), S["stem"], "stem")
    h = F.max_pool2d(h, 3, 2, 1)
    s_in = S["stem"]
    for i, blk in enumerate(bb.blocks):
        idt, s_res = h, s_in
        if blk.down is not None:
            s_res = S[f"b{i}.down"]
            idt = close(quant.int8_conv_codes(blk.down, h, s_in, s_res), s_res, f"b{i}.down")
        t1 = close(quant.int8_conv_codes(blk.conv1, h, s_in, S[f"b{i}.c1"]), S[f"b{i}.c1"], f"b{i}.c1")
        t2 = close(quant.int8_conv_codes(blk.conv2, t1, S[f"b{i}.c1"], S[f"b{i}.c2"]), S[f"b{i}.c2"], f"b{i}.c2")
        h = close(quant.int8_conv_codes(blk.conv3, t2, S[f"b{i}.c2"], S[f"b{i}.out"], idt, s_res, act="relu"),
                  S[f"b{i}.out"], f"b{i}.out")
        s_in = S[f"b{i}.out"]
    outs = [close(quant.int8_conv_codes(br, h, s_in, S["aspp.cat"]), S["aspp.cat"], f"aspp.{j}")
            for j, br in enumerate([a.b0] + list(a.atrous))]
    with torch.no_grad():  # the fp32 pooling branch, an input of the projection
        pooled = a.pool(F.adaptive_avg_pool2d(h * s_in, 1))
        pw, _ = a.project.fold()
        ncat = len(outs) * a.cout
        img_bias = F.conv2d(pooled, pw[:, ncat:]).flatten(1)
    wq, sw, b = quant._qw(a.project)
    v = I.exact_conv(torch.cat(outs, 1), wq[:, :ncat], sw, b, S["aspp.cat"], img_bias=img_bias, act="relu")
    proj = close(I.requant(v, S["aspp.proj"]), S["aspp.proj"], "aspp.proj")
    assert next(it, None) is None  # every quantisation point of the replay was visited
    # the logits: an fp32 sum of K = 256 terms is within K * 2^-24 * sum |terms| of the exact one
    lq, ls, lb = quant._qw(model.logits)
    ref = I.exact_conv(proj, lq, ls, lb, S["aspp.proj"])
    mag = I.exact_conv(proj.abs(), lq.abs(), ls, lb.abs(), S["aspp.proj"])
    assert bool(((logits.double() - ref).abs() <= 260 * 2.0 ** -24 * mag).all())


def test_pack_int8_layout_scale_and_slice():
    """``pack_int8``: weights [Cout, kh, kw, Cin] int8, scale = s_w * s_in, and a channel
    slice (the ASPP projection without its pooling columns) keeps the per-channel scale of
    the FULL filter, as ``fake_quant_forward`` quantises it."""
    layer = _layer(48, 24, 3, seed=9)
    wq, sw, b = quant._qw(layer)
    w8, sc, bi = quant.pack_int8(layer, 0.037, "cpu")
    assert w8.dtype == torch.int8 and tuple(w8.shape) == (24, 3, 3, 48) and w8.is_contiguous()
    for o, ky, kx, c in ((0, 0, 0, 0), (5, 1, 2, 17), (23, 2, 0, 47)):
        assert int(w8[o, ky, kx, c]) == int(wq[o, c, ky, kx])
    assert torch.equal(w8.permute(0, 3, 1, 2).float(), wq)
    assert torch.equal(sc, (sw * 0.037).float()) and torch.equal(bi, b)
    proj = _layer(40, 8, 1, seed=10)
    with torch.no_grad():  # channel 0's largest weight sits in the columns that are cut off
        proj.conv.weight[0, 39] = 4.0 * proj.conv.weight[0].abs().max()
    wq, sw, b = quant._qw(proj)
    w8, sc, _ = quant.pack_int8(proj, 0.5, "cpu", wslice=slice(0, 32))
    assert tuple(w8.shape) == (8, 1, 1, 32)
    assert torch.equal(w8[:, 0, 0, :].float(), wq[:, :32, 0, 0])
    assert torch.equal(sc, (sw * 0.5).float())
    assert int(w8[0].abs().max()) < 127 and int(wq[0].abs().max()) == 127  # not rescaled to the slice


def test_q_rounds_half_to_even_and_clamps():
    t = torch.tensor([0.5, 1.5, 2.5, -0.5, -1.5, 126.5, 127.5, 300.0, -300.0])
    assert quant.q(t, 1.0).tolist() == [0.0, 2.0, 2.0, -0.0, -2.0, 126.0, 127.0, 127.0, -127.0]
    assert quant.q(t * 0.25, 0.25).tolist() == [v * 0.25 for v in quant.q(t, 1.0).tolist()]


def test_calibrate_scales_cover_every_quantisation_point():
    from semantic_segmentation_server_amd.models.deeplab import build_model, synthetic_normalized
    model = build_model("resnet50", 19, calibrate_hw=33).float().eval()
    x = synthetic_normalized(1, 33, 33, torch.Generator().manual_seed(2))
    S = quant.calibrate(model, x)
    want = {"stem", "aspp.cat", "aspp.proj"}
    for i, blk in enumerate(model.backbone.blocks):
        want |= {f"b{i}.c1", f"b{i}.c2", f"b{i}.out"} | ({f"b{i}.down"} if blk.down is not None else set())
    assert set(S) == want and all(v > 0 for v in S.values())
    with torch.no_grad():
        stem = model.backbone.stem(x)
    assert S["stem"] == pytest.approx(float(stem.abs().max()) / 127.0, rel=1e-6)


def test_code_comparator():
    """The comparator of the GPU int8 tests: one code two steps off fails, 0.2 % of the codes
    one step off fails, 0.05 % one step off passes; the bf16 bound is elementwise."""
    g = torch.Generator().manual_seed(1)
    ref = torch.randint(-100, 101, (2, 50, 40, 25), generator=g, dtype=torch.int32)
    n = ref.numel()

    def off(count, by):
        t = ref.clone().flatten()
        t[torch.randperm(n, generator=g)[:count]] += by
        return t.view_as(ref).to(torch.int8)

    assert I.assert_codes_close(ref.to(torch.int8), ref, "same") == (0.0, 0)
    with pytest.raises(AssertionError, match="2 steps"):
        I.assert_codes_close(off(1, 2), ref, "two")
    with pytest.raises(AssertionError, match="one"):
        I.assert_codes_close(off(n // 500, 1), ref, "one")
    share, mx = I.assert_codes_close(off(n // 2000, -1), ref, "few")
    assert mx == 1 and share == pytest.approx(5e-4)
    v = torch.randn(1000, generator=g).double() * 8
    I.assert_bf16_close(v.to(torch.bfloat16), v, "bf16")
    bad = v.to(torch.bfloat16).clone()
    bad[7] = bad[7] * (1 + 2.0 ** -6)
    with pytest.raises(AssertionError, match="bf16 bound"):
        I.assert_bf16_close(bad, v, "bf16")
    bad[7] = float("nan")
    with pytest.raises(AssertionError, match="non-finite"):
        I.assert_bf16_close(bad, v, "bf16")


def test_stem_pixel_table_forms():
    """The two ways to normalise a pixel: ``reference_ops.preprocess`` rounds p * (1 / 127.5)
    and then the subtraction, the stem kernels' fused multiply-add rounds once
    (``int8_ref.stem_pixel_table``). 158 of the 256 values differ, by an fp32 ulp of 1, and
    exactly one rounds to a different bf16 -- the MFMA stems' operand."""
    from semantic_segmentation_server_amd.ops import reference_ops as R
    p = torch.arange(256, dtype=torch.uint8)
    two = R.preprocess(p.view(1, 1, 256, 1).expand(1, 1, 256, 3).contiguous(), torch.arange(256),
                       torch.zeros(1, dtype=torch.long))[0, 0, 0]
    one = I.stem_pixel_table()
    assert torch.equal(two, p.float() * torch.tensor(1.0 / 127.5, dtype=torch.float32) - 1.0)
    assert int((one != two).sum()) == 158
    assert float((one.double() - two.double()).abs().max()) <= 2.0 ** -23  # an ulp of the product
    assert int((one.to(torch.bfloat16) != two.to(torch.bfloat16)).sum()) == 1
    assert one[0] == -1.0  # the letterbox padding
    # through the letterbox gather the two-rounding table IS preprocess
    g = torch.Generator().manual_seed(3)
    frames = torch.randint(0, 256, (2, 12, 16, 3), generator=g, dtype=torch.uint8)
    lx, ly, *_ = R.letterbox_luts(16, 12, 33, 33)
    assert torch.equal(I.letterbox_pixels(frames, torch.tensor(lx.tolist()), torch.tensor(ly.tolist()), two),
                       R.preprocess(frames, lx, ly))


@pytest.fixture(scope="module")
def exact_plan():
    """A ``HipDeepLabInt8`` plan built on the CPU (no kernel runs, no autotuning) at 321^2,
    B = 2, portrait camera, its buffers filled with what exact kernels would leave."""
    import numpy as np
    from semantic_segmentation_server_amd import config as C
    from semantic_segmentation_server_amd.models.deeplab import build_model
    from semantic_segmentation_server_amd.models.hip_int8 import HipDeepLabInt8
    from semantic_segmentation_server_amd.ops import reference_ops as R
    from semantic_segmentation_server_amd.runtime.sources import SyntheticSource
    S, B, cw, ch = 321, 2, 150, 200
    model = build_model("resnet50", 19, calibrate_hw=65)
    lx, ly, *_ = R.letterbox_luts(cw, ch, S, S)
    f, _, _ = SyntheticSource(cw, ch, pool=B, seed=13).read_batch(B)
    frames = torch.from_numpy(np.array(f))
    scales = quant.calibrate(model.float(), R.preprocess(frames, lx, ly))
    cfg = C.Config(arch="resnet50", dtype="int8", input_size=S, batch=B, backend="hip", graph=False,
                   num_classes=19)
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(HipDeepLabInt8, "_autotune", lambda self, *a: setattr(self, "choices", {}))
        hm = HipDeepLabInt8(model, torch.device("cpu"), cfg, scales=scales)
        ops, bufs = hm._plan(B, ch, cw)
    I.fill_from_references(hm, ops, bufs, frames, lx, ly)
    return hm, ops, bufs, frames, lx, ly


def test_plan_walker_on_exact_buffers(exact_plan):
    """The walker of the GPU plan tests, on a plan whose buffers hold the exact results: its
    step list mirrors the plan (op count and types), every step passes with zero mismatch,
    and the conditions on the inputs hold (no saturation, live ASPP branches)."""
    hm, ops, bufs, frames, lx, ly = exact_plan
    rep = I.check_plan(hm, ops, bufs, frames, lx, ly, run=False)
    assert len(rep) == 2 + 16 * 3 + 4 + 2 and all(r[2] == 0.0 and r[3] == 0 for r in rep)
    assert sorted(n for n in bufs if any(sel(n) for sel in I.STAGES.values())) == \
        sorted(s[1] for s in I.plan_steps(hm))
    only = I.check_plan(hm, ops, bufs, frames, lx, ly, run=False, select=I.STAGES["aspp_head"])
    assert [r[0] for r in only] == ["aspp_cat", "aspp_proj"]


def _mutated(bufs, name, value):
    saved = bufs[name].clone()
    bufs[name].copy_(value)
    return saved


def test_plan_walker_sees_a_wrong_dilation(exact_plan):
    """Rate 17 instead of 18 in the last ASPP branch (21 x 21 maps: off-centre taps are
    live) fails the ASPP step and nothing else."""
    import copy
    hm, ops, bufs, frames, lx, ly = exact_plan
    br = copy.deepcopy(hm.model.aspp.atrous[-1])
    assert br.dilation == 18
    br.dilation = 17
    x = bufs["r15_out"].permute(0, 3, 1, 2).float()
    wrong = quant.int8_conv_codes(br, x, hm.s_feat, hm.scales["aspp.cat"], act="relu")
    cat = bufs["aspp_cat"].clone()
    cat[..., 3 * hm.A:] = wrong.permute(0, 2, 3, 1).to(torch.int8)
    saved = _mutated(bufs, "aspp_cat", cat)
    try:
        with pytest.raises(AssertionError, match="aspp_cat"):
            I.check_plan(hm, ops, bufs, frames, lx, ly, run=False, select=lambda n: n == "aspp_cat")
    finally:
        bufs["aspp_cat"].copy_(saved)


def test_plan_walker_sees_a_shared_image_bias(exact_plan):
    """Image 0's pooled bias applied to every image fails the projection step."""
    hm, ops, bufs, frames, lx, ly = exact_plan
    wq, sw, b = quant._qw(hm.model.aspp.project)
    ib = bufs["img_bias"][:1].expand_as(bufs["img_bias"])
    v = I.exact_conv(bufs["aspp_cat"].permute(0, 3, 1, 2).float(), wq[:, :hm.cat_c], sw, b,
                     hm.scales["aspp.cat"], img_bias=ib, act="relu")
    saved = _mutated(bufs, "aspp_proj", I.requant(v, hm.scales["aspp.proj"]).permute(0, 2, 3, 1).to(torch.int8))
    try:
        with pytest.raises(AssertionError, match="aspp_proj"):
            I.check_plan(hm, ops, bufs, frames, lx, ly, run=False, select=lambda n: n == "aspp_proj")
    finally:
        bufs["aspp_proj"].copy_(saved)


def test_plan_walker_sees_logits_padding_and_label_errors(exact_plan):
    hm, ops, bufs, frames, lx, ly = exact_plan
    saved = bufs["logits"].clone()
    try:
        bufs["logits"][0, 3, 4, hm.num_classes] = 1.0  # a write into the row padding
        with pytest.raises(AssertionError, match="padding"):
            I.check_plan(hm, ops, bufs, frames, lx, ly, run=False, select=lambda n: n == "logits")
        bufs["logits"].copy_(saved)
        bufs["logits"][1, 0, 0, 5] = saved[1, 0, 0, 5].float() * 1.0625 + 0.01  # one logit off by 6 %
        with pytest.raises(AssertionError, match="bf16 bound"):
            I.check_plan(hm, ops, bufs, frames, lx, ly, run=False, select=lambda n: n == "logits")
    finally:
        bufs["logits"].copy_(saved)
    lab = bufs["labels"].clone()
    try:
        bufs["labels"][0, :2] = 255
        with pytest.raises(AssertionError, match="label agreement"):
            I.check_plan(hm, ops, bufs, frames, lx, ly, run=False, select=lambda n: n == "labels")
    finally:
        bufs["labels"].copy_(lab)


def _poisoned_walk(exact_plan, wrong):
    """``check_plan(chip_poison=...)`` over the projection and the logits of the exact plan with
    host ops (``int8_ref.reference_ops``), ``wrong(name, write, hidden, calls)`` wrapping the
    picked op of each. The poison callable NaN-fills ``hidden``, the stand-in for on-chip state."""
    hm, ops, bufs, frames, lx, ly = exact_plan
    sel = lambda n: n in ("aspp_proj", "logits")  # noqa: E731
    hops = I.reference_ops(hm, ops, bufs, frames, lx, ly, only=sel)
    hidden, calls = torch.zeros(1), [0]
    for op, (_, name, _) in zip(hops, I.plan_steps(hm)):
        if sel(name):
            vname, (write,) = op.variants[op.pick]
            op.variants[op.pick] = (vname, [wrong(name, write, hidden, calls)])
    saved = {n: bufs[n].clone() for n in ("aspp_proj", "logits")}
    try:
        return I.check_plan(hm, hops, bufs, frames, lx, ly, run=True, every_variant=False, select=sel,
                            chip_poison=lambda: hidden.fill_(float("nan")))
    finally:
        for n, t in saved.items():
            bufs[n].copy_(t)


def test_poisoned_walk_passes_on_clean_ops(exact_plan):
    rep = _poisoned_walk(exact_plan, lambda name, write, hidden, calls: write)
    assert [r[0] for r in rep] == ["aspp_proj", "logits"]


def test_poisoned_walk_sees_stale_state_and_a_call_counter(exact_plan):
    """An op that adds a hidden host tensor (NaN once poisoned, cleared by the op as a kernel
    overwrites its LDS) is reported as P != A at its buffer and variant; one that adds its call
    count as not reproducible."""
    hm, ops = exact_plan[:2]
    pick = {op.name: op.variants[op.pick][0] for op in ops if hasattr(op, "variants")}
    names = {name: op.name for op, (_, name, _) in zip(ops, I.plan_steps(hm)) if hasattr(op, "variants")}

    def stale(name, write, hidden, calls):
        def op(*a):
            write(*a)
            if name == "logits":
                t = exact_plan[2][name]
                t[0, 1, 2, 3] = t[0, 1, 2, 3].float() + hidden[0]
            hidden.zero_()  # every kernel leaves its own bytes behind
        return op
    with pytest.raises(AssertionError) as err:
        _poisoned_walk(exact_plan, stale)
    lines = str(err.value).splitlines()[1:]
    assert len(lines) == 1 and lines[0].startswith(f"logits/{pick[names['logits']]}: the poisoned run differs: P != A "
                                                   "at 1 of ") and lines[0].endswith("first at (0, 1, 2, 3)"), lines

    def counter(name, write, hidden, calls):
        def op(*a):
            write(*a)
            if name == "aspp_proj":
                calls[0] += 1
                exact_plan[2][name][1, 0, 0, 0] = calls[0]
        return op
    with pytest.raises(AssertionError) as err:
        _poisoned_walk(exact_plan, counter)
    lines = str(err.value).splitlines()[1:]
    assert any(ln.startswith(f"aspp_proj/{pick[names['aspp_proj']]}: not reproducible: A' != A at 1 of ") and
               ln.endswith("first at (1, 0, 0, 0)") for ln in lines), lines
    assert all(ln.startswith("aspp_proj/") for ln in lines), lines
