"""The teacher-forced walker of the bf16 plans (``models/hip_model.HipDeepLab``).

Shared by tests/test_bf16_plan.py (the plans on the device: every step, every variant of every
``Choice``) and tests/test_plan_bound_cpu.py (the walker itself: emulated plans pass, injected
faults are reported at their buffer). Imported the way tests/int8_ref.py is.

``plan_steps`` describes what ``HipDeepLab._build`` emits, from the model's specs alone; the
walker asserts that the description and the ops agree in length and in their Choice / plain-op
pattern. Every variant name maps to a reference FAMILY by its prefix (``family``): a name
without one is an error, so no kernel family enters a plan without a reference. The references
are the float64 ``(v, e)`` pairs of tests/bound_cases.py, computed on the CPU from the step's
input AS THE DEVICE LEFT IT (nothing accumulates across steps), once per (step, family) and
per distinct input image, and compared where the buffer lives, at every element.

Before a variant runs, every buffer it writes is NaN (labels: 255); after it, every element of
every such buffer lies within its bound, the logits' padding channels are all untouched or all
zero, the ticket buffers are all zero again and the guard bands (``SSA_GUARD_BYTES``) intact.
The fp32 split-K / split-hidden partial buffers are NaN-filled too but have no reference of
their own: how a sum is cut is the kernel's business, its total is checked in the output.

``chip_poison=<callable>`` turns the walk into a reproducibility walk that needs no reference:
every leaf call of every variant at any depth runs three times on the buffers its sub-step
writes (outputs, fp32 partials; the ticket counters are compared too): A and A' from NaN-filled
buffers, P from NaN-filled buffers after ``chip_poison()`` (tests/chip_poison.py: every CU's LDS
and every SIMD's registers NaN). A != A' is "not reproducible", P != A names buffer, variant,
the count of differing elements and the first index; the tickets and guard bands are checked
after P. What A is worth is the business of the walks above: the same calls on the same inputs
are held to their float64 bounds there.

``dw_chain_fp16`` is exact in float64 only below 2^5; the BN-folded depthwise operands of these
models pass it (sum |h w| + |b| reaches 56 from the operands alone and 44 on the test frames in
blocks 11-16), so the chain carries the 2^-53 relative term its docstring describes.
"""
from __future__ import annotations

import os
import re
from types import SimpleNamespace as NS
from typing import Callable, Dict, List, Optional

import numpy as np
import torch
import torch.nn.functional as F

import bound_cases as BC
import chip_poison as CP
import upsample_ref as UR

MIN_LIVE = 0.25  # least share of a clamped reference that must lie strictly inside the clamp
CLAMP = {"relu": (0.0, float("inf")), "relu6": (0.0, 6.0), "unit": (0.0, 1.0)}
UPSAMPLE_FIELDS = (("noise", 7), ("smooth", 7))  # upsample_ref.make_logits fields and seeds


class PlanCheckError(AssertionError):
    """Every failed check of one walk; ``failures`` = [(buffer, variant, message)]."""

    def __init__(self, failures):
        self.failures = failures
        super().__init__(f"{len(failures)} plan checks failed:\n" + "\n".join(m for _, _, m in failures))


# ---------------------------------------------------------------- families
_FAMILIES = {  # choice kind -> (variant name prefix, family), first match wins
    "block": (("slice", "band"), ("band", "band"), ("stream", "span"), ("tile", "tile"), ("fused", "row"),
              ("unfused", "unfused"), ("dwproj", "dwproj"), ("dwp", "dwp")),
    "stem+block0": (("stem_band", "stem_block0"), ("stem_block0_", "stem_block0"), ("separate", "separate")),
    "stem": (("fp32", "stem_fp32"), ("mfmaw", "stem_mfma")),
    "pw": (("gemm", "mat"), ("pw", "mat")),
    "rate": (("tapg", "conv"), ("tap", "conv"), ("v4g", "conv"), ("v5g", "conv"), ("v6g", "conv"), ("v4", "conv")),
    "aspp.branches": (("grouped_v", "grouped"), ("separate", "separate")),
    "aspp.head": (("head_g", "head"), ("split", "split")),
    "aspp.proj": (("v3", "mat"), ("v4", "mat"), ("v5", "mat"), ("v6", "mat")),
    "upsample": (("rows", "labels"), ("lane", "labels"), ("union", "labels"), ("cand", "labels")),
}


def choice_kind(cname: str) -> str:
    if re.fullmatch(r"block\d+", cname):
        return "block"
    if re.fullmatch(r"block\d+\.expand|aspp\.b0|logits", cname):
        return "pw"
    if re.fullmatch(r"aspp\.rate\d+", cname):
        return "rate"
    if cname in _FAMILIES:
        return cname
    raise AssertionError(f"choice {cname!r} has no reference families")


def family(cname: str, vname: str) -> str:
    """The reference family of variant ``vname`` of choice ``cname``; none is an error."""
    for prefix, fam in _FAMILIES[choice_kind(cname)]:
        if vname.startswith(prefix):
            return fam
    raise AssertionError(f"{cname}/{vname}: a variant without a reference family")


def combines_in_launch(vname: str) -> bool:
    """The variants whose launch combines its own partials through the ticket counters."""
    return vname.endswith("+pool") or bool(re.search(r"(h\d+|k\d+)c(\+pool)?$", vname))


# ---------------------------------------------------------------- layouts
def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _nhwc(pair):
    v, e = pair
    return v.permute(0, 2, 3, 1), None if e is None else e.permute(0, 2, 3, 1)


def _rows(t):
    """[R, h, w, C] -> [R h w, C]."""
    return t.reshape(-1, t.shape[-1])


def _unrows(pair, like):
    v, e = pair
    shp = tuple(like.shape[:-1]) + (v.shape[-1],)
    return v.reshape(shp), None if e is None else e.reshape(shp)


def _dense(packed):
    """(w [Cout, Cin, k, k] bf16, b) of ``hip_model._pack_dense``'s (w [Cout, k, k, Cin], b)."""
    w, b = packed
    return w.detach().cpu().permute(0, 3, 1, 2).contiguous(), b.detach().cpu()


def _dw(packed):
    w, b = packed  # [9, C] fp32
    w = w.detach().cpu()
    return w.t().reshape(w.shape[1], 1, 3, 3).contiguous(), b.detach().cpu()


def _stem_w(hm):
    sw, sb, sk, ss, sact, sc = hm.stem
    assert ss == 2, "stem_bound is a stride-2 conv"
    return sw.detach().cpu().reshape(sk, sk, 3, sc).permute(3, 2, 0, 1).contiguous(), sb.detach().cpu(), sact


# ---------------------------------------------------------------- the step list
def _ref(key, inputs, fn, emu=None):
    """One reference: ``fn(inp) -> [(buffer, channel slice or None, (v, e), clamp or None)]``
    from the CPU copies ``inp`` of the named inputs (leading dimension: distinct images), the
    pairs in the buffer's layout; ``emu(inp, order) -> [(buffer, slice, tensor)]``: what a
    correct kernel of the family leaves there."""
    return NS(key=key, inputs=list(inputs), fn=fn, emu=emu)


def _sub(writes, refs=(), choice=None, scratch=()):
    """One op of a variant: the buffers it writes, its references, and the nested ``Choice``
    the op may be (``pw_choice`` returns a plain op where ``pw_conv`` does not apply)."""
    return NS(writes=list(writes), refs=list(refs), choice=choice, scratch=list(scratch))


def _pw_ref(key, xname, out, w, b, *, act=None, fmt="bf16", res=None, img=None, sl=None):
    """A 1x1 conv as rows x weights (``mat_bound``): conv_gemm k = 1, pw_conv."""
    inputs = [xname] + ([res] if res else []) + ([img] if img else [])

    def args(inp):
        x = inp[xname]
        kw = dict(act=act, fmt=fmt)
        if res:
            kw["res"] = _rows(inp[res])
        if img:
            kw["img_rows"] = inp[img].double().repeat_interleave(x.shape[1] * x.shape[2], 0)
        return x, kw

    def fn(inp):
        x, kw = args(inp)
        return [(out, sl, _unrows(BC.mat_bound(_rows(x), w, b, **kw), x), act)]

    def emu(inp, order):
        x, kw = args(inp)
        if kw.get("img_rows") is not None:
            kw["img_rows"] = kw["img_rows"].float()
        return [(out, sl, _unrows((BC.mat_emulate(_rows(x), w, b, order=order, **kw), None), x)[0])]
    return _ref(key, inputs, fn, emu)


def _conv_ref(key, xname, out, w, b, *, stride=1, dil=1, act=None, res=None, groups=1, sl=None):
    inputs = [xname] + ([res] if res else [])
    kw = dict(stride=stride, dil=dil, act=act, groups=groups)

    def fn(inp):
        r = _nchw(inp[res]) if res else None
        return [(out, sl, _nhwc(BC.conv_bound(_nchw(inp[xname]), w, b, res=r, **kw)), act)]

    def emu(inp, order):
        r = _nchw(inp[res]) if res else None
        return [(out, sl, _nhwc((BC.conv_emulate(_nchw(inp[xname]), w, b, res=r, order=order, **kw), None))[0])]
    return _ref(key, inputs, fn, emu)


def plan_steps(hm, B: int, Hc: int, Wc: int) -> List[NS]:
    """The ordered description of what ``HipDeepLab._build`` emits for (B, camera), from the
    model's specs: per top-level op ``NS(name, choice, ...)``; ``name`` is the Choice's name or,
    for a plain op, the buffer it writes; ``subs(vname)`` the ops of a variant."""
    from semantic_segmentation_server_amd.ops import hip_ops as K
    from semantic_segmentation_server_amd.ops import reference_ops as R
    from semantic_segmentation_server_amd.ops.hip_ops import conv_out_hw
    assert not hm.confidence, "the confidence plan's final op is tests/test_confidence_gpu.py's"
    assert os.environ.get("SSA_POOL_FORK", "0") != "1", "the side-stream fork is not a plan step"
    H, W = hm.H, hm.W
    sw, sb, sk, ss, sact, sc = hm.stem
    stem_w, stem_b, _ = _stem_w(hm)
    h, w = conv_out_hw(H, W, sk, ss, 1)
    steps: List[NS] = []

    lut_x, lut_y, *_ = R.letterbox_luts(Wc, Hc, W, H)  # the letterbox of the plan's camera

    def pixels(inp, bf16):
        return BC.stem_pixels(inp["frames"], lut_x, lut_y, bf16)

    def stem_ref(form):
        bf = form == "stem_mfma"

        def fn(inp):
            return [("stem", None, _nhwc(BC.stem_bound(pixels(inp, bf), stem_w, stem_b, act=sact, bf16_weights=bf)), sact)]

        def emu(inp, order):
            wk = stem_w.to(torch.bfloat16) if bf else stem_w
            return [("stem", None, BC.conv_emulate(pixels(inp, bf), wk, stem_b, stride=2, act=sact, order=order)
                     .permute(0, 2, 3, 1))]
        return _ref(("stem", form), ["frames"], fn, emu)

    # -------------------------------------------------- MobileNetV2 block
    def block_subs(i, xname, vname):
        blk = hm.blocks[i]
        s = blk["spec"]
        out, exp, dwb, e16 = f"b{i}_out", f"b{i}_exp", f"b{i}_dw", f"b{i}_exp16"
        fam = family(f"block{i}", vname)
        res = xname if s.residual else None
        wd, bd = _dw(blk["dw"])
        pwd, pbd = _dense(blk["project"])
        scratch = [f"b{i}_part"]

        def fused(P, tile, key):
            def fn(inp):
                return [(out, None, _nhwc(BC.fused_ir_bound(_nchw(inp[xname]), P, tile=tile)), None)]

            def emu(inp, order):
                Pc = {k: (v.detach().cpu() if torch.is_tensor(v) else v) for k, v in P.items()}
                return [(out, None, BC.fused_ir_emulate(_nchw(inp[xname]), Pc, tile=tile, order=order)
                         .permute(0, 2, 3, 1))]
            return [_sub([out], [_ref((f"block{i}", key), [xname], fn, emu)], scratch=scratch)]

        # (the numpy re-executions ``fused_band.emulate_fused_band`` / ``fused_span.emulate_fused_span``
        # round the depthwise product and its sum separately, twice per tap where the kernels'
        # fma rounds once: they miss the chain's e = 0 elements by an fp16 ulp of the hidden
        # value. The emulation of these families is ``fused_ir_emulate`` on the operands
        # unpacked from the same blob, which rounds each fma once.)
        if fam == "band":
            return fused(BC.unpack_fused_band(hm._packed(blk, "band"), s.stride, s.residual), True, "band")
        if fam == "span":
            assert re.fullmatch(r"stream(\d+)(g|wr3|w|r3)?(L)?(?:h(\d+)(c)?)?", vname), \
                f"block{i}/{vname}: not a stream variant name"
            return fused(dict(BC.unpack_fused_span(hm._packed(blk, "span")), dil=s.dilation, residual=s.residual),
                         True, "span")
        if fam == "tile":
            return fused(blk["fused_tile"], True, "tile")
        if fam == "row":
            return fused(blk["fused"], False, "row")
        # the families that keep the expansion in memory
        subs = []
        if blk["expand"] is not None:
            ew, eb = _dense(blk["expand"])
            ew = ew[:, :, 0, 0]
        if fam in ("unfused", "dwproj") and blk["expand"] is not None:
            subs.append(_sub([exp], [_pw_ref((f"block{i}", "expand"), xname, exp, ew, eb, act="relu6")],
                             choice=f"block{i}.expand"))
        hin = exp if blk["expand"] is not None else xname
        if fam == "unfused":
            subs.append(_sub([dwb], [_conv_ref((f"block{i}", "dw"), hin, dwb, wd, bd, stride=s.stride,
                                               dil=s.dilation, act="relu6", groups=wd.shape[0])]))
            subs.append(_sub([out], [_conv_ref((f"block{i}", "proj"), dwb, out, pwd, pbd, res=res)]))
            return subs
        if fam == "dwproj":
            dpw, dpb = (t.detach().cpu()[:s.cout] for t in blk["dwproj"])
            inputs = [exp] + ([res] if res else [])

            def fn(inp):
                r = _nchw(inp[res]) if res else None
                return [(out, None, _nhwc(BC.dw_project_bound(_nchw(inp[exp]), wd, bd, dpw, dpb, stride=s.stride,
                                                             dil=s.dilation, res=r)[1]), None)]

            def emu(inp, order):
                r = _nchw(inp[res]) if res else None
                d = BC.conv_emulate(_nchw(inp[exp]), wd, bd, stride=s.stride, dil=s.dilation, act="relu6",
                                    groups=wd.shape[0], order=order)
                return [(out, None, BC.conv_emulate(d, dpw[:, :, None, None], dpb, res=r, order=order).permute(0, 2, 3, 1))]
            subs.append(_sub([out], [_ref((f"block{i}", "dwproj"), inputs, fn, emu)]))
            return subs
        assert fam == "dwp"
        subs.append(_sub([e16], [_pw_ref((f"block{i}", "pw16"), xname, e16, ew, eb, act="relu6", fmt="fp16")]))
        wp16 = pwd[:, :, 0, 0]
        Pd = dict(Cin=s.hidden, Cout=s.cout, stride=s.stride, dil=s.dilation, hidP=s.hidden, we=None, residual=False,
                  wd_h=wd.reshape(-1, 9).t().half(), bd_h=bd.half(), wp_h=wp16.float().half(), bp=pbd)
        inputs = [e16] + ([res] if res else [])

        def fn(inp):
            r = _nchw(inp[res]) if res else None
            return [(out, None, _nhwc(BC.dw_proj_fused_bound(_nchw(inp[e16]), wd, bd, wp16, pbd, stride=s.stride,
                                                            dil=s.dilation, res=r)), None)]

        def emu(inp, order):
            r = _nchw(inp[res]) if res else None
            return [(out, None, BC.fused_ir_emulate(_nchw(inp[e16]), Pd, tile=True, order=order, res=r)
                     .permute(0, 2, 3, 1))]
        subs.append(_sub([out], [_ref((f"block{i}", "dwpf"), inputs, fn, emu)]))
        return subs

    def block_step(i, xname):
        return NS(name=f"block{i}", choice=True, subs=lambda v, i=i, xname=xname: block_subs(i, xname, v))

    # -------------------------------------------------- backbone
    if hm.kind == "mnv2":
        first = 0
        if hm.stem_block0 is not None:
            first = 1
            P0 = hm.stem_block0

            def sb0_subs(vname):
                if family("stem+block0", vname) == "separate":
                    return [_sub(["stem"], [stem_ref("stem_fp32")]), _sub(["b0_dw", "b0_out"], choice="block0")]

                def fn(inp):
                    return [("b0_out", None, _nhwc(BC.stem_block0_bound(pixels(inp, True), P0)), None)]

                def emu(inp, order):
                    return [("b0_out", None, BC.stem_block0_emulate(pixels(inp, True), P0, order).permute(0, 2, 3, 1))]
                return [_sub(["b0_out"], [_ref(("stem+block0", "fused"), ["frames"], fn, emu)])]
            steps.append(NS(name="stem+block0", choice=True, subs=sb0_subs,
                            nested={"block0": lambda v: block_subs(0, "stem", v)}))
        else:
            steps.append(NS(name="stem", choice=False, sub=_sub(["stem"], [stem_ref("stem_fp32")])))
        x, c = "stem", sc
        for i, blk in enumerate(hm.blocks):
            s = blk["spec"]
            if i >= first:
                steps.append(block_step(i, x))
            h, w = conv_out_hw(h, w, 3, s.stride, s.dilation)
            x, c = f"b{i}_out", s.cout
    else:
        if (sc, sk) == (64, 7):
            steps.append(NS(name="stem", choice=True, subs=lambda v: [_sub(["stem"], [stem_ref(family("stem", v))])]))
        else:
            steps.append(NS(name="stem", choice=False, sub=_sub(["stem"], [stem_ref("stem_fp32")])))

        def pool_fn(inp):
            return [("pool0", None, _nhwc(BC.maxpool_bound(_nchw(inp["stem"]))), None)]

        def pool_emu(inp, order):
            return [("pool0", None, F.max_pool2d(_nchw(inp["stem"]).float(), 3, 2, 1).permute(0, 2, 3, 1))]
        steps.append(NS(name="pool0", choice=False,
                        sub=_sub(["pool0"], [_ref(("pool0", "max"), ["stem"], pool_fn, pool_emu)])))
        h, w = conv_out_hw(h, w, 3, 2, 1)
        x, c = "pool0", sc
        for i, blk in enumerate(hm.blocks):
            m = blk["blk"]
            convs = [(f"r{i}_c1", x, blk["conv1"], 1, 1, "relu", None),
                     (f"r{i}_c2", f"r{i}_c1", blk["conv2"], m.stride, m.dilation, "relu", None)]
            idt = x
            if blk["down"] is not None:
                idt = f"r{i}_down"
                convs.append((idt, x, blk["down"], m.stride, 1, None, None))
            convs.append((f"r{i}_out", f"r{i}_c2", blk["conv3"], 1, 1, "relu", idt))
            for name, src, packed, st, dl, act, res in convs:
                wc, bc = _dense(packed)
                steps.append(NS(name=name, choice=False, sub=_sub([name], [_conv_ref(
                    (name, "conv"), src, name, wc, bc, stride=st, dil=dl, act=act, res=res)])))
            h, w = conv_out_hw(h, w, 3, m.stride, m.dilation)
            x, c = f"r{i}_out", m.conv3.cout

    # -------------------------------------------------- ASPP branches and the pooling branch
    A, cat_c = hm.aspp_c, hm.cat_c
    branches = [(_dense(hm.aspp_b0), 1)] + [(_dense(p), r) for p, r in hm.aspp_atrous]
    brefs = [_conv_ref(("aspp", f"branch{j}"), x, "aspp_cat", wj, bj, dil=r, act="relu", sl=slice(j * A, (j + 1) * A))
             for j, ((wj, bj), r) in enumerate(branches)]
    pool_subs, item = [], False
    if hm.has_pool:
        w1, b1, w2 = hm.pool_w.detach().cpu(), hm.pool_b.detach().cpu(), hm.proj_pool_w.detach().cpu()
        if c <= 2048 and A <= 512 and c % 8 == 0 and A % 4 == 0:
            def ib_fn(inp, xn=x):
                return [("img_bias", None, BC.aspp_pool_bound(_nchw(inp[xn]), w1, b1, w2), None)]

            def ib_emu(inp, order, xn=x):
                gap = _nchw(inp[xn]).float().mean((2, 3))
                return [("img_bias", None, torch.relu(gap @ w1.t() + b1) @ w2.t())]
            ibref = _ref(("aspp", "img_bias"), [x], ib_fn, ib_emu)
            pool_subs = [_sub(["img_bias"], [ibref])]
            item = os.environ.get("SSA_POOL_FUSED", "1") != "0"
        else:  # the matvec fall-back: global_avgpool, two matvecs
            def gap_fn(inp, xn=x):
                v, e = BC.gap_bound(_nchw(inp[xn]))
                return [("gap", None, (v, e), None)]
            pool_subs = [
                _sub(["gap"], [_ref(("aspp", "gap"), [x], gap_fn, lambda inp, o, xn=x: [
                    ("gap", None, _nchw(inp[xn]).float().mean((2, 3)))])]),
                _sub(["pooled"], [NS(key=("aspp", "pooled"), inputs=["gap"], fn=lambda inp: [
                    ("pooled", None, BC.mat_bound(inp["gap"], w1, b1, act="relu", fmt=None), "relu")],
                    emu=lambda inp, o: [
                        ("pooled", None, BC.mat_emulate(inp["gap"], w1, b1, act="relu", fmt=None, order=o))])]),
                _sub(["img_bias"], [NS(key=("aspp", "img_bias"), inputs=["pooled"], fn=lambda inp: [
                    ("img_bias", None, BC.mat_bound(inp["pooled"], w2, None, fmt=None), None)],
                    emu=lambda inp, o: [("img_bias", None, BC.mat_emulate(inp["pooled"], w2, None, fmt=None, order=o))])])]

    def sep_subs():
        return [_sub([("aspp_cat", slice(0, A))], [brefs[0]], choice="aspp.b0")] + \
            [_sub([("aspp_cat", slice((j + 1) * A, (j + 2) * A))], [brefs[j + 1]], choice=f"aspp.rate{r}")
             for j, (_, r) in enumerate(hm.aspp_atrous)]

    if len(hm.aspp_atrous) <= 3 and c % 8 == 0:
        fused = item and any(K.pool_item_fits(gv, c, A) for gv in (5, 6, 8, 12, 13, 14, 15, 16, 17, 18)
                             if gv in K.GROUP_POOL_VARIANTS)

        def br_subs(vname, fused=fused):
            tail = pool_subs if fused else []
            if family("aspp.branches", vname) == "separate":
                return sep_subs() + tail
            if vname.endswith("+pool"):
                assert fused, vname
                return [_sub(["aspp_cat", "img_bias"], brefs + pool_subs[0].refs, scratch=["aspp_part"])]
            return [_sub(["aspp_cat"], brefs, scratch=["aspp_part"])] + tail
        steps.append(NS(name="aspp.branches", choice=True, subs=br_subs, nested={}))
        if not fused:
            steps += [NS(name=s_.writes[0], choice=False, sub=s_) for s_ in pool_subs]
    else:
        for s_ in sep_subs():
            ischoice = s_.choice != "aspp.b0" or (K.pw_supported(c, A) and cat_c % 8 == 0)
            steps.append(NS(name=s_.choice if ischoice else "aspp_cat", choice=ischoice, sub=s_,
                            subs=lambda v, s_=s_: [_sub(s_.writes, s_.refs)]))
        steps += [NS(name=s_.writes[0], choice=False, sub=s_) for s_ in pool_subs]

    # -------------------------------------------------- head
    ncls, ldk = hm.num_classes, hm.ldk
    pw_, pb_ = hm.proj_w.detach().cpu(), hm.proj_b.detach().cpu()
    lw, lb = hm.logit_w.detach().cpu().reshape(ncls, -1), hm.logit_b.detach().cpu()
    img = "img_bias" if hm.has_pool else None
    cls = slice(0, ncls)
    proj_sub = _sub(["aspp_proj"], [_pw_ref(("head", "proj"), "aspp_cat", "aspp_proj", pw_, pb_, act="relu", img=img)],
                    choice="aspp.proj")
    logit_sub = _sub(["logits"], [_pw_ref(("head", "logits"), "aspp_proj", "logits", lw, lb, sl=cls)], choice="logits")
    logits_choice = K.pw_supported(A, ldk) and ldk % 8 == 0
    if A == 256 and cat_c == 1024 and ncls <= 32 and ldk <= 32:
        inputs = ["aspp_cat"] + ([img] if img else [])

        def args(inp):
            cat = inp["aspp_cat"]
            rows = inp[img].double().repeat_interleave(cat.shape[1] * cat.shape[2], 0) if img else None
            return cat, rows

        def head_fn(inp):
            cat, rows = args(inp)
            return [("logits", cls, _unrows(BC.aspp_head_bound(_rows(cat), pw_, pb_, lw, lb, rows), cat), None)]

        def head_emu(inp, order):
            cat, rows = args(inp)
            proj = BC.mat_emulate(_rows(cat), pw_, pb_, act="relu", img_rows=None if rows is None else rows.float(),
                                  order=order)
            lg = BC.mat_emulate(proj, lw, lb, order=order)
            return [("logits", None, F.pad(lg, (0, ldk - ncls)).reshape(tuple(cat.shape[:-1]) + (ldk,)))]
        href = _ref(("head", "fused"), inputs, head_fn, head_emu)

        def head_subs(vname):
            if family("aspp.head", vname) == "split":
                return [proj_sub, logit_sub]
            return [_sub(["logits"], [href])]
        steps.append(NS(name="aspp.head", choice=True, subs=head_subs))
    else:
        steps.append(NS(name="aspp.proj", choice=True, sub=proj_sub, subs=lambda v: [_sub(proj_sub.writes, proj_sub.refs)]))
        steps.append(NS(name="logits", choice=logits_choice, sub=logit_sub,
                        subs=lambda v: [_sub(logit_sub.writes, logit_sub.refs)]))
    steps.append(NS(name="upsample", choice=True, subs=None, geom=(h, w)))
    for st in steps:
        st.nested = getattr(st, "nested", {})
    return steps


def nested_subs(step, cname: str, sub, vname: str):
    """The ops of variant ``vname`` of a Choice nested in a variant of ``step``."""
    if cname in step.nested:
        return step.nested[cname](vname)
    family(cname, vname)  # a name without a family is an error
    return [_sub(sub.writes, sub.refs)]


# ---------------------------------------------------------------- comparison
def within(got: torch.Tensor, v: torch.Tensor, e: torch.Tensor, what: str) -> float:
    """The rule of ``bound_ref.assert_within``, evaluated where the buffer lives (one
    implementation for the CPU tier and the device): |got - v| <= e at EVERY element, a
    non-finite ``got`` fails, a reference that is not finite or a bound that is not a finite
    non-negative number is an error. Returns max |got - v| / e; names the worst index."""
    assert got.shape == v.shape == e.shape, (what, tuple(got.shape), tuple(v.shape), tuple(e.shape))
    assert bool(torch.isfinite(v).all()), f"{what}: the reference v is not finite"
    assert bool(torch.isfinite(e).all()) and bool((e >= 0).all()), f"{what}: the bound e is not finite or negative"
    g = got.double()
    d = (g - v).abs()
    d = torch.where(torch.isfinite(g), d, torch.full_like(d, float("inf")))
    bad = d > e
    ratio = torch.where(d == 0, torch.zeros_like(d), d / e)
    worst = float(ratio.max()) if ratio.numel() else 0.0
    if bool(bad.any()):
        flat = int(torch.where(bad, ratio, torch.full_like(ratio, -1.0)).argmax())
        idx = tuple(int(i) for i in np.unravel_index(flat, tuple(v.shape)))
        raise AssertionError(
            f"{what}: {int(bad.sum())} of {bad.numel()} elements outside their bound; worst at {idx}: "
            f"got {float(g[idx])!r}, v {float(v[idx])!r}, e {float(e[idx])!r}; max |got - v| / e = {worst:.4g}")
    return worst


def label_ref(logits, K, H, W):
    """``upsample_ref.label_ref`` with the margin scaled to the logits' magnitude: MARGIN
    presumes |logit| <= 32 (the fp32 lerps err in proportion). One image at a time: the float64
    interpolant of 32 maps of 513^2 x 21 is 1.4 GB. Returns (argmax, decided mask, scale)."""
    scale = max(1.0, float(logits[..., :K].float().abs().max()) / 32.0)
    per = [UR.label_ref(logits[b:b + 1], K, H, W, margin=UR.MARGIN * scale) for b in range(logits.shape[0])]
    return torch.cat([a for a, _ in per]), torch.cat([m for _, m in per]), scale


# ---------------------------------------------------------------- the walker
class Walker:
    def __init__(self, hm, ops, bufs, frames, lx, ly, *, run=True, every_variant=True, select=None, cache=None,
                 upsample_fields=True, families=None, chip_poison=None):
        B, Hc, Wc = (int(v) for v in frames.shape[:3])
        from semantic_segmentation_server_amd.ops import reference_ops as R
        want = R.letterbox_luts(Wc, Hc, hm.W, hm.H)[:2]  # the references letterbox as the plan's camera does
        assert all(np.array_equal(np.asarray(torch.as_tensor(a).cpu()), np.asarray(b)) for a, b in zip((lx, ly), want))
        self.hm, self.ops, self.bufs, self.args = hm, ops, bufs, (frames, lx, ly)
        self.run, self.every, self.select = run, every_variant, select
        self.steps = plan_steps(hm, B, Hc, Wc)
        self.cache: Dict[tuple, tuple] = {} if cache is None else cache
        self.failures: List[tuple] = []
        self.report: List[tuple] = []  # (buffer, variant, max ratio, flip share)
        self.fields, self.families = upsample_fields, families
        self.chip_poison, self.leaves = chip_poison, 0  # leaf calls that ran A / A' / P
        assert chip_poison is None or run, "the reproducibility walk runs the ops"
        self.dev = bufs["labels"].device

    # ---- inputs, references
    def _input(self, name):
        return self.args[0] if name == "frames" else self.bufs[name]

    def reference(self, ref):
        """The checks of ``ref`` on the device, for the inputs as they are now: from the cache
        while the inputs are bit-equal to those it was computed from; per distinct image."""
        ins = [self._input(n) for n in ref.inputs]
        hit = self.cache.get(ref.key)
        if hit is not None and all(a.shape == b.shape and torch.equal(a, b) for a, b in zip(hit[0], ins)):
            return hit[1]
        B = ins[0].shape[0]
        reps, which = [], []
        for b in range(B):
            r = next((k for k, rb in enumerate(reps) if all(torch.equal(t[b], t[rb]) for t in ins)), None)
            if r is None:
                r = len(reps)
                reps.append(b)
            which.append(r)
        inp = {n: t[reps].detach().cpu() for n, t in zip(ref.inputs, ins)}
        idx = torch.tensor(which, device=self.dev)
        checks = []
        for buf, sl, (v, e), clamp in ref.fn(inp):
            v = v.double()
            e = torch.zeros_like(v) if e is None else e.double()
            live = None
            if clamp is not None:
                lo, hi = CLAMP[clamp]
                live = ((v > lo) & (v < hi)).double().mean().item()
            checks.append((buf, sl, v.to(self.dev)[idx].contiguous(), e.to(self.dev)[idx].contiguous(), live))
        self.cache[ref.key] = ([t.clone() for t in ins], checks)
        return checks

    def _check(self, sub, what):
        for ref in sub.refs:
            try:
                checks = self.reference(ref)
            except AssertionError as err:
                self.failures.append((ref.key[0], what, f"{ref.key}/{what}: {err}"))
                continue
            for buf, sl, v, e, live in checks:
                name = f"{buf}/{what}" + ("" if sl is None else f"[{sl.start}:{sl.stop}]")
                got = self.bufs[buf] if sl is None else self.bufs[buf][..., sl]
                try:
                    assert live is None or live >= MIN_LIVE, \
                        f"{name}: only {live:.3f} of the reference lies strictly inside its clamp"
                    ratio = within(got, v, e, name)
                    flips = (e > 0).double().mean().item()
                    print(f"[bound] {name}: max |got - v| / e = {ratio:.3f}, flip possible at {flips:.3e}")
                    self.report.append((buf, what, ratio, flips))
                except AssertionError as err:
                    self.failures.append((buf, what, str(err)))
                if buf == "logits":
                    self._check_pad(what)

    def _check_pad(self, what):
        pad = self.bufs["logits"][..., self.hm.num_classes:].float()
        if pad.numel() and not (bool(torch.isnan(pad).all()) or bool((pad == 0).all())):
            at = tuple(int(i) for i in (~((pad == 0) | torch.isnan(pad))).nonzero()[0])
            self.failures.append(("logits", what, f"logits/{what}: the padding channels {self.hm.num_classes}.. are "
                                  f"neither all untouched nor all zero; first at {at}: {float(pad[at])!r}"))

    def _check_state(self, what):
        for name, t in self.bufs.items():
            if t.dtype == torch.int32 and re.fullmatch(r"(b\d+|aspp)_cnt\d*", name) and bool((t != 0).any()):
                self.failures.append((name, what, f"{name}/{what}: {int((t != 0).sum())} tickets are not zero again"))
        for name, raw, guard, nb in self.hm._guards:
            g = torch.cat([raw[:guard], raw[guard + nb:]])
            if bool((g != 0x5A).any()):
                at = int((g != 0x5A).nonzero()[0])
                self.failures.append((name, what, f"{name}/{what}: guard band overwritten, first at byte "
                                      f"{at - guard if at < guard else at - guard + nb} of the buffer"))

    # ---- running
    def _poison(self, names):
        for n in names:
            n, sl = n if isinstance(n, tuple) else (n, None)
            t = self.bufs.get(n)
            if t is not None:
                (t if sl is None else t[..., sl]).fill_(255 if t.dtype == torch.uint8 else float("nan"))

    def _sync(self):
        if self.dev.type == "cuda":
            torch.cuda.synchronize()

    def _variants(self, op):
        if not self.run or not self.every:
            return [op.variants[op.pick]]
        return op.variants

    # ---- the reproducibility walk (``chip_poison``)
    def _tickets(self):
        return [n for n, t in self.bufs.items() if t.dtype == torch.int32 and re.fullmatch(r"(b\d+|aspp)_cnt\d*", n)]

    def _repro(self, call, names, what):
        """A, A', P of one leaf call on the buffers ``names`` it writes (module docstring)."""
        fill = list(names)
        seen = []
        for n in [n[0] if isinstance(n, tuple) else n for n in fill] + self._tickets():
            if n in self.bufs and n not in seen:
                seen.append(n)
        snaps = []
        for run in ("A", "A'", "P"):
            self._poison(fill)
            if run == "P":
                self.chip_poison()
            call(*self.args)
            self._sync()
            if run != "P":
                snaps.append([self.bufs[n].clone() for n in seen])
        self.leaves += 1
        clean = True
        for i, n in enumerate(seen):
            for tag, a, b in (("not reproducible: A' != A", snaps[0][i], snaps[1][i]),
                              ("the poisoned run differs: P != A", snaps[0][i], self.bufs[n])):
                d = CP.bit_diff(a, b)
                if d is not None:
                    clean = False
                    self.failures.append((n, what, f"{n}/{what}: {tag} at {d[0]} of {a.numel()} elements, "
                                          f"first at {d[1]}"))
        self.report.append((names[0][0] if isinstance(names[0], tuple) else names[0], what, 0.0, 0.0))
        return clean

    def _walk_choice(self, step, op, subs_of):
        from semantic_segmentation_server_amd.models.plan import Choice
        if self.chip_poison is not None:
            return self._walk_choice_poisoned(step, op, subs_of)
        for vname, calls in self._variants(op):
            fam = family(op.name, vname)  # a name without a family is an error
            if self.families is not None and op.name == step.name and fam not in self.families:
                continue
            what = vname if op.name == step.name else f"{op.name}={vname}"
            for _ in range(2 if self.run and combines_in_launch(vname) else 1):
                subs = subs_of(vname)
                assert len(subs) == len(calls), f"{op.name}/{vname}: {len(calls)} ops, {len(subs)} described"
                if self.run:
                    self._poison([n for s in subs for n in s.writes + s.scratch])
                for call, sub in zip(calls, subs):
                    if isinstance(call, Choice):
                        assert call.name == sub.choice, (call.name, sub.choice)
                        self._walk_choice(step, call, lambda v, c=call, s=sub: nested_subs(step, c.name, s, v))
                        continue
                    assert sub.refs, f"{op.name}/{vname}: a plain op where the nested choice {sub.choice} is expected"
                    if self.run:
                        call(*self.args)
                        self._sync()
                    self._check(sub, what)
                if self.run and len(subs) > 1:  # the whole variant once more: a later op spoiled nothing
                    for sub in subs:
                        self._check(sub, what)
                self._check_state(what)

    def _walk_choice_poisoned(self, step, op, subs_of):
        from semantic_segmentation_server_amd.models.plan import Choice
        for vname, calls in self._variants(op):
            fam = family(op.name, vname)
            if self.families is not None and op.name == step.name and fam not in self.families:
                continue
            what = vname if op.name == step.name else f"{op.name}={vname}"
            subs = subs_of(vname)
            assert len(subs) == len(calls), f"{op.name}/{vname}: {len(calls)} ops, {len(subs)} described"
            for call, sub in zip(calls, subs):
                if isinstance(call, Choice):
                    assert call.name == sub.choice, (call.name, sub.choice)
                    self._walk_choice_poisoned(step, call, lambda v, c=call, s=sub: nested_subs(step, c.name, s, v))
                    continue
                assert sub.refs, f"{op.name}/{vname}: a plain op where the nested choice {sub.choice} is expected"
                self._repro(call, sub.writes + sub.scratch, what)
            self._check_state(what)

    def _walk_upsample_poisoned(self, step, op):
        """Every upsample variant A / A' / P on the plan's logits and on the noise and smooth
        fields: the label maps bit-equal."""
        bufs = self.bufs
        h, w = step.geom
        B, K, ldk = bufs["logits"].shape[0], self.hm.num_classes, self.hm.ldk
        inputs = [("plan", None)]
        if self.fields:
            inputs += [(f, UR.make_logits(B, h, w, K, ldk, f, seed)) for f, seed in UPSAMPLE_FIELDS]
        saved = bufs["logits"].clone()
        for tag, lg in inputs:
            if lg is not None:
                bufs["logits"].copy_(lg.to(self.dev))
            for vname, calls in self._variants(op):
                family("upsample", vname)

                def call(*args, calls=calls):
                    for c in calls:
                        c(*args)
                self._repro(call, ["labels"], f"{tag}/{vname}")
                self._check_state(vname)
        if len(inputs) > 1:
            bufs["logits"].copy_(saved)
            op(*self.args)
            self._sync()

    def _walk_upsample(self, step, op):
        if self.chip_poison is not None:
            return self._walk_upsample_poisoned(step, op)
        hm, bufs = self.hm, self.bufs
        h, w = step.geom
        B, K, ldk = bufs["logits"].shape[0], hm.num_classes, hm.ldk
        inputs = [("plan", None)]
        if self.run and self.fields:
            inputs += [(f, UR.make_logits(B, h, w, K, ldk, f, seed)) for f, seed in UPSAMPLE_FIELDS]
        saved = bufs["logits"].clone()
        for tag, lg in inputs:
            if lg is not None:
                bufs["logits"].copy_(lg.to(self.dev))
            arg, ok, scale = label_ref(bufs["logits"], K, hm.H, hm.W)
            undecided = 1.0 - ok.double().mean().item()
            classes = int(arg.unique().numel())
            if undecided > UR.MAX_UNDECIDED:
                self.failures.append(("labels", tag, f"labels/{tag}: {undecided:.2e} of the pixels are undecided "
                                      f"(margin {UR.MARGIN * scale:.1e})"))
            for vname, calls in self._variants(op):
                family("upsample", vname)
                if self.run:
                    self._poison(["labels"])
                    for call in calls:
                        call(*self.args)
                    self._sync()
                wrong = (bufs["labels"].long() != arg) & ok
                print(f"[labels] {tag}/{vname}: {classes} classes, undecided {undecided:.2e}, margin scale {scale:.1f}")
                if bool(wrong.any()):
                    at = tuple(int(i) for i in wrong.nonzero()[0])
                    self.failures.append(("labels", vname, f"labels/{vname} ({tag} logits): {int(wrong.sum())} decided "
                                          f"pixels differ from the float64 argmax; first at {at}: got "
                                          f"{int(bufs['labels'][at])}, expected {int(arg[at])}"))
                self._check_state(vname)
                self.report.append(("labels", f"{tag}/{vname}", 0.0, undecided))
        if len(inputs) > 1:
            bufs["logits"].copy_(saved)
            if self.run:
                op(*self.args)
                self._sync()

    def structure(self, deep: bool = True) -> int:
        """The description against the ops, launching nothing: the length, the Choice / plain-op
        pattern and the choices' names; ``deep``: also every variant of every
        choice at any depth: a family for its name, one described op per op, the nested choices
        where they are expected. Returns the number of variants seen."""
        from semantic_segmentation_server_amd.models.plan import Choice
        pattern = [isinstance(op, Choice) for op in self.ops]
        assert len(self.ops) == len(self.steps), (len(self.ops), [s.name for s in self.steps])
        assert pattern == [s.choice for s in self.steps], \
            [(s.name, s.choice, p) for s, p in zip(self.steps, pattern) if s.choice != p]
        seen = 0

        def variants(step, op, subs_of):
            nonlocal seen
            for vname, calls in op.variants:
                family(op.name, vname)
                seen += 1
                if subs_of is None:
                    continue
                subs = subs_of(vname)
                assert len(subs) == len(calls), f"{op.name}/{vname}: {len(calls)} ops, {len(subs)} described"
                for call, sub in zip(calls, subs):
                    if isinstance(call, Choice):
                        assert call.name == sub.choice, (call.name, sub.choice)
                        variants(step, call, lambda v, c=call, s=sub: nested_subs(step, c.name, s, v))
                    else:
                        assert sub.refs, f"{op.name}/{vname}: a plain op where the choice {sub.choice} is expected"

        for op, step in zip(self.ops, self.steps):
            if step.choice:
                assert op.name == step.name, (op.name, step.name)
                if deep:
                    variants(step, op, step.subs)
        return seen

    def walk(self):
        self.structure(deep=False)
        for op, step in zip(self.ops, self.steps):
            if self.select is not None and not self.select(step.name):
                if self.run:
                    op(*self.args)
                continue
            if step.name == "upsample":
                self._walk_upsample(step, op)
            elif step.choice:
                self._walk_choice(step, op, step.subs)
            elif self.chip_poison is not None:
                self._repro(op, step.sub.writes + step.sub.scratch, "op")
                self._check_state("op")
            else:
                if self.run:
                    self._poison(step.sub.writes)
                    op(*self.args)
                    self._sync()
                self._check(step.sub, "op")
                self._check_state("op")
        if self.failures:
            raise PlanCheckError(self.failures)
        return self.report


def check_plan(hm, ops, bufs, frames, lx, ly, **kw) -> List[tuple]:
    """Walk a ``HipDeepLab`` plan in order (module docstring). ``run``: execute the ops, a
    ``Choice`` through every variant (``every_variant``) or its pick alone, nested choices
    likewise, variants with an in-launch combine twice; the last variant's output feeds the next
    step. ``run=False``: check ``bufs`` as a finished run of the picks left them. ``select(step
    name)``: the steps to check, the others are only executed; ``families``: of their top-level
    variants, only those of these reference families (a stage split per family). ``cache``: references shared
    between walks (reused only while a step's inputs are bit-equal). ``chip_poison``: the
    reproducibility walk of the module docstring instead of the references. Returns [(buffer, variant,
    max |got - v| / e, flip share)]; raises ``PlanCheckError`` naming every failed check."""
    return Walker(hm, ops, bufs, frames, lx, ly, **kw).walk()


def worst(report):
    return max(report, key=lambda r: r[2])


# ---------------------------------------------------------------- emulated plans (run=False)
def _emulate(wk, sub, order):
    for ref in sub.refs:
        inp = {n: wk._input(n).detach().cpu() for n in ref.inputs}
        for buf, sl, t in ref.emu(inp, order):
            dst = wk.bufs[buf] if sl is None else wk.bufs[buf][..., sl]
            dst.copy_(t.to(dst.dtype))


def emulated_ops(hm, ops, bufs, frames, lx, ly, order: str = "whole") -> list:
    """The plan's ops with every leaf call, of every variant at any depth, replaced by a host
    function that writes what a correct kernel of its family leaves in the buffers (as
    ``fill_from_emulation`` does): a plan that ``check_plan(run=True)`` can walk on the CPU, into
    which a test injects a wrong op by replacing one callable."""
    from semantic_segmentation_server_amd.models.plan import Choice
    from semantic_segmentation_server_amd.ops import reference_ops as R
    wk = Walker(hm, ops, bufs, frames, lx, ly, run=False)

    def leaf(sub):
        return lambda *args: _emulate(wk, sub, order)

    def choice(step, op, subs_of):
        variants = []
        for vname, calls in op.variants:
            subs = subs_of(vname)
            assert len(subs) == len(calls), f"{op.name}/{vname}: {len(calls)} ops, {len(subs)} described"
            variants.append((vname, [
                choice(step, c, lambda v, c=c, s=s: nested_subs(step, c.name, s, v)) if isinstance(c, Choice) else leaf(s)
                for c, s in zip(calls, subs)]))
        new = Choice(op.name, variants)
        new.pick = op.pick
        return new

    def upsample(*args):
        lg = _nchw(bufs["logits"][..., :hm.num_classes]).float()
        bufs["labels"].copy_(R.upsample_argmax(lg, hm.H, hm.W))

    out = []
    for op, step in zip(ops, wk.steps):
        if step.name == "upsample":
            new = Choice(op.name, [(vname, [upsample]) for vname, _ in op.variants])
            new.pick = op.pick
            out.append(new)
        elif step.choice:
            out.append(choice(step, op, step.subs))
        else:
            out.append(leaf(step.sub))
    return out


def fill_from_emulation(hm, ops, bufs, frames, lx, ly, order: str = "whole",
                        fault: Optional[Callable] = None, select: Optional[Callable] = None) -> None:
    """Write into ``bufs`` what a correct kernel of each PICKED family would leave there, each
    step computed from the buffers before it (fp32 accumulation in ``order``, roundings where
    the family's reference has them). ``fault(step name, bufs, redo)`` is called after each step
    is written and may damage its buffers (``redo()`` emulates the step again): the later steps
    are then computed from the damaged ones, as a plan with one wrong kernel would.
    ``select(step name)``: the steps to write (their inputs are whatever ``bufs`` holds)."""
    from semantic_segmentation_server_amd.models.plan import Choice
    from semantic_segmentation_server_amd.ops import reference_ops as R
    wk = Walker(hm, ops, bufs, frames, lx, ly, run=False)

    def emulate(sub):
        _emulate(wk, sub, order)

    def do_choice(step, op, subs_of):
        vname, calls = op.variants[op.pick]
        for call, sub in zip(calls, subs_of(vname)):
            if isinstance(call, Choice):
                do_choice(step, call, lambda v, c=call, s=sub: nested_subs(step, c.name, s, v))
            else:
                emulate(sub)

    for op, step in zip(ops, wk.steps):
        if select is not None and not select(step.name):
            continue
        if step.name == "upsample":
            def redo():
                lg = _nchw(bufs["logits"][..., :hm.num_classes]).float()
                bufs["labels"].copy_(R.upsample_argmax(lg, hm.H, hm.W))
        elif step.choice:
            redo = lambda op=op, step=step: do_choice(step, op, step.subs)  # noqa: E731
        else:
            redo = lambda step=step: emulate(step.sub)  # noqa: E731
        redo()
        if fault is not None:
            fault(step.name, bufs, redo)
