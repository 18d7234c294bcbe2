"""The shapes of the bounded kernel goldens and their float64 references (tests/bound_ref.py).

tests/test_hip_kernels.py takes its parametrisations and references from here, and
tests/test_bound_ref_cpu.py runs the same shapes through fp32 emulations, so the two tiers
cannot drift apart. Every reference states where the kernel it stands for rounds.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

import bound_ref as BR

# B, H, W, Cin, Cout, k, stride, dil, act, res, ldo_pad, co_off  (test_conv_gemm)
CONV_GEMM = [
    (2, 17, 19, 16, 96, 1, 1, 1, "relu6", False, 0, 0),
    (2, 17, 19, 24, 24, 1, 1, 1, None, True, 0, 0),
    (1, 33, 33, 320, 256, 1, 1, 1, "relu", False, 0, 0),
    (1, 33, 33, 160, 960, 1, 1, 1, "relu6", False, 0, 0),
    (2, 33, 33, 256, 21, 1, 1, 1, None, False, 3, 0),
    (1, 33, 33, 320, 256, 3, 1, 6, "relu", False, 512, 256),
    (1, 33, 33, 320, 256, 3, 1, 12, "relu", False, 0, 0),
    (1, 33, 33, 320, 256, 3, 1, 18, "relu", False, 0, 0),
    (2, 21, 23, 64, 64, 3, 2, 1, "relu", False, 0, 0),
    (2, 21, 23, 64, 256, 1, 2, 1, None, False, 0, 0),
    (3, 9, 11, 8, 40, 3, 1, 2, "relu", False, 0, 0),
    (2, 33, 33, 960, 160, 1, 1, 1, None, True, 0, 0),
    (2, 33, 33, 96, 576, 1, 1, 1, "relu6", False, 0, 0),
    (2, 65, 65, 144, 32, 1, 1, 1, None, False, 0, 0),
    (1, 33, 33, 1024, 256, 1, 1, 1, "relu", False, 0, 0),
]
TAP_GROUPED = [(3, 33, 33, 6), (2, 33, 33, 12), (2, 33, 33, 18), (2, 17, 21, 24)]  # B, H, W, rate
GROUPED_ASPP = [  # B, H, W, Cin, Cout, variant
    (3, 33, 33, 320, 256, 5), (2, 33, 33, 320, 256, 6), (2, 17, 19, 64, 200, 8),
    (2, 21, 20, 96, 136, 11), (3, 33, 33, 320, 256, 12), (2, 17, 19, 96, 200, 13),
    (2, 21, 20, 320, 136, 14), (3, 33, 33, 320, 256, 15), (2, 21, 20, 96, 136, 16),
    (3, 33, 33, 320, 256, 17), (2, 21, 20, 96, 136, 18)]
GROUPED_SPLITK = [(1, 18, 2), (1, 17, 4), (1, 5, 6), (2, 18, 6), (3, 17, 3)]  # B, variant, ks
ASPP_BRANCHES = ((1, 1), (3, 6), (3, 12), (3, 18))  # k, rate
TAP_CONV = [  # B, H, W, Cin, Cout, rate, grouped
    (3, 33, 33, 320, 256, 6, True), (2, 33, 33, 320, 256, 12, False), (2, 33, 33, 320, 256, 18, True),
    (2, 17, 21, 160, 96, 24, True), (1, 9, 11, 64, 200, 1, False), (2, 20, 20, 256, 136, 2, True)]
PW_CONV = [  # M, Cin, Cout, act, res, img, ldo_pad, co_off, n_out
    (2 * 33 * 33, 160, 960, "relu6", False, False, 0, 0, None),   # b14-16 expansion
    (1000, 96, 576, "relu6", False, False, 0, 0, None),           # M tail (not a multiple of 128/256)
    (777, 24, 144, "relu6", False, False, 0, 0, None),            # K = 24 (< one 32-deep step)
    (1089, 320, 256, "relu", False, False, 1024, 256, None),      # ASPP b0 into a concat slice
    (1089, 256, 21, None, False, False, 0, 0, 24),                # logits, N padded 21 -> 24
    (999, 64, 96, None, True, False, 0, 0, None),                 # residual
    (4 * 121, 128, 80, "relu", False, True, 0, 0, None),          # per-image bias, N % 64 != 0
]
PW_FP16 = (1500, 96, 576)  # M, Cin, Cout (test_pw_conv_fp16_out)
DEPTHWISE = [  # B, H, W, C, stride, dil
    (2, 33, 35, 96, 1, 1), (2, 33, 35, 96, 2, 1), (1, 33, 33, 960, 1, 2), (2, 257, 257, 32, 1, 1),
    (1, 65, 65, 144, 2, 1)]
DW_PROJECT = [  # hid, cout, stride, dil, res
    (576, 96, 1, 1, True), (576, 160, 1, 1, False), (960, 160, 1, 2, True), (960, 320, 1, 2, False),
    (384, 64, 2, 1, False)]
MATVEC = [(8, 256, 2048, True), (9, 37, 2048, False), (1, 40, 64, True), (3, 19, 30, True)]  # B, N, K, bias
ASPP_POOL = [(3, 33, 33, 320, 256), (2, 17, 13, 2048, 256), (1, 9, 7, 40, 24)]  # B, h, w, C, N


def _conv(stride, pad, dil, groups=1):
    return lambda x, w: F.conv2d(x, w, None, stride, pad, dil, groups)


def _matmul(x, w):
    return x @ w.t()


# ---------------------------------------------------------------- references
def conv_bound(x, w, b, *, stride=1, dil=1, act=None, res=None, img_bias=None, groups=1, fmt="bf16",
               x_err=None):
    """conv_gemm, tap_conv, the grouped / split-K ASPP GEMMs, depthwise3x3. NCHW x, w
    [Cout, Cin / groups, k, k]. Rounding points: none inside (fp32 accumulators of
    n = Cin / groups * k * k products, in whatever order; split-K adds fp32 partials), then
    bias, per-image bias and residual in fp32, the activation, and ONE rounding to ``fmt``."""
    k = w.shape[-1]
    extras = [(b[None, :, None, None], None)]
    if img_bias is not None:
        extras.append((img_bias[:, :, None, None], None))
    if res is not None:
        extras.append((res, None))
    p = BR.linear(_conv(stride, dil * (k // 2), dil, groups), (x, x_err), w, w.shape[1] * k * k, extras)
    p = BR.act(p, act)
    return BR.round_stage(p[0], p[1], fmt) if fmt else p


def mat_bound(x, w, b, *, act=None, res=None, img_rows=None, fmt="bf16", x_err=None):
    """pw_conv, bias_act, matvec: rows of x [M, K] against w [N, K]. As ``conv_bound``: fp32
    accumulation of n = K products, fp32 epilogue, activation, one rounding (``fmt`` None: an
    fp32 output, no rounding)."""
    extras = []
    if b is not None:
        extras.append((b[None, :], None))
    if img_rows is not None:
        extras.append((img_rows, None))
    if res is not None:
        extras.append((res, None))
    p = BR.linear(_matmul, (x, x_err), w, w.shape[1], extras)
    p = BR.act(p, act)
    return BR.round_stage(p[0], p[1], fmt) if fmt else p


def bias_act_bound(x, b, img_rows, act):
    """bias_act: act(x + bias + per-image bias) of a bf16 x: three fp32 terms (the linear
    stage with n = 1 and an identity weight), one rounding to bf16."""
    one = torch.ones(1, 1, dtype=torch.float64)
    extras = [(b[None, :], None)] + ([(img_rows, None)] if img_rows is not None else [])
    p = BR.linear(lambda v, w: v * w, (x, None), one, 1, extras)
    p = BR.act(p, act)
    return BR.round_stage(p[0], p[1], "bf16")


def dw_project_bound(x, wd, bd, wp_bf16, bp, *, stride, dil, res=None):
    """dw_project. Rounding points (dw_proj.hip / model_ops.hip): the depthwise 3 x 3 runs in
    fp32 (9 products + bias), ReLU6, and is rounded to bf16 as the projection's MFMA operand;
    the projection accumulates hid products in fp32, adds bias and the bf16 residual, and
    rounds once to bf16. Returns (hidden pair, output pair)."""
    hid = conv_bound(x, wd, bd, stride=stride, dil=dil, act="relu6", groups=x.shape[1])
    B, C, OH, OW = hid[0].shape
    rows = lambda t: None if t is None else t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])
    out = mat_bound(rows(hid[0]), wp_bf16, bp, res=rows(res), x_err=rows(hid[1]))
    back = lambda t: None if t is None else t.reshape(B, OH, OW, -1).permute(0, 3, 1, 2)
    return hid, (back(out[0]), back(out[1]))


MAXPOOL = [(2, 33, 35, 64), (1, 8, 9, 24), (3, 1, 5, 8)]  # B, H, W, C


def maxpool_bound(x):
    """maxpool3x3s2 (3 x 3 window, stride 2, pad 1; the padding never wins): a maximum of bf16
    values is one of them. No arithmetic and no rounding: e is None (exact), NCHW x."""
    return F.max_pool2d(x.double(), 3, 2, 1), None


def gap_bound(x):
    """global_avgpool (fp32 output, no rounding to a narrow format): per channel an fp32 sum
    of the HW bf16 values of x [B, C, h, w] in any order, times 1 / HW."""
    B, C, h, w_ = x.shape
    hw = h * w_
    inv = torch.full((hw,), 1.0 / hw, dtype=torch.float64)
    return BR.linear(lambda v, w: v.reshape(B, C, hw) @ w, (x, None), inv, hw)


def aspp_pool_bound(x, w1, b1, w2):
    """aspp_pool (fp32 throughout, no rounding to a narrow format): the mean of HW bf16
    values per channel (a sum of HW terms times 1 / HW), relu(W1 gap + b1) over C terms,
    W2 pooled over N terms. x [B, C, h, w]."""
    C = x.shape[1]
    gap = gap_bound(x)
    pooled = BR.act(BR.linear(_matmul, gap, w1, C, [(b1[None, :], None)]), "relu")
    return BR.linear(_matmul, pooled, w2, w2.shape[1])


def _tap_views(t, k, stride, dil):
    """The k * k shifted (strided) views of the zero-padded NCHW tensor, in tap order."""
    pad = dil * (k // 2)
    H, W = t.shape[-2:]
    OH = (H + 2 * pad - dil * (k - 1) - 1) // stride + 1
    OW = (W + 2 * pad - dil * (k - 1) - 1) // stride + 1
    tp = F.pad(t, (pad, pad, pad, pad))
    for i in range(k):
        for j in range(k):
            yield tp[:, :, i * dil:i * dil + (OH - 1) * stride + 1:stride,
                     j * dil:j * dil + (OW - 1) * stride + 1:stride]


def dw_chain_fp16(x, wd_h, bd_h, *, stride, dil, act="relu6", bias_last=False):
    """The packed-fp16 depthwise of the tile kernels (fused_ir.hip ``fused_ir_tile_kernel``,
    fused_ir_stream.hip): the accumulator starts at the fp16 bias (bias first) and takes the
    nine taps in raster order, each ``d = fma(x, w, d)`` rounded to fp16 (v_pk_fma_f16: the
    product is exact, one rounding per tap), then a [0, 6] clamp. A rounding stage per tap;
    e only grows by e_x |w| as long as float64 holds d + x w exactly. Every fp16 number is
    a multiple of 2^-24, so every term is a multiple of 2^-48 and the sum is exact in float64
    while it stays below 2^5, as it does at the kernel tests' magnitudes (hidden values in
    [0, 6], weights of order one). It is not exact in general: under a larger d the sum spans
    more than 53 bits and float64 rounds it before the fp16 rounding. The BN-folded depthwise
    weights of the plan tests reach that (sum |x w| + |b| up to 44 in MobileNetV2's blocks
    11-16), so where |d + x w| >= 2^5 that 2^-53 relative term is added to e before the
    rounding stage; below 2^5 nothing changes.

    ``bias_last`` (fused_ir_band.hip, fused_ir_slice.hip): the accumulator of an output row
    starts at zero, takes the taps of its three input rows as they stream by (ky outer, kx
    inner: raster order again; a tap on the zero padding adds an exact zero, so skipping it
    changes nothing), and the bias is added last, ``d = D + bd`` rounded to fp16, then clamped."""
    v, e = x
    C = v.shape[1]
    w = wd_h.double().reshape(C, 9)
    bias = bd_h.double()[None, :, None, None]
    acc = torch.zeros((), dtype=torch.float64) if bias_last else bias
    err = None
    xe = None if e is None else list(_tap_views(e.double(), 3, stride, dil))
    for t, xv in enumerate(_tap_views(v.double(), 3, stride, dil)):
        wt = w[:, t][None, :, None, None]
        acc = acc + xv * wt
        if xe is not None:
            err = xe[t] * wt.abs() + (0.0 if err is None else err)
        acc, err = BR.round_stage(acc, _f64_slack(acc, err), "fp16")
    if bias_last:
        acc = acc + bias
        acc, err = BR.round_stage(acc, _f64_slack(acc, err), "fp16")
    return BR.act((acc, err), act)


def _f64_slack(acc, err):
    """``err`` plus float64's own rounding of a chain sum that is no longer exact (>= 2^5)."""
    big = acc.abs() >= 32.0
    if not bool(big.any()):
        return err
    slack = torch.where(big, acc.abs() * 2.0 ** -53, torch.zeros_like(acc))
    return slack if err is None else err + slack


def dw_fp16_loose(x, wd_h, bd_h, *, stride, dil, act="relu6", bias_last=False):
    """A packed-fp16 depthwise WITHOUT resets: the minimum every band, slice and stem kernel
    must meet, whatever its tap and bias order (tests/test_bound_ref_cpu.py checks that the
    flip-aware chains lie inside it). Whatever the order, and whether or not a
    multiply and its add are fused, at most 19 results are rounded to fp16 (9 products, 9 sums,
    the bias), each a partial sum no larger than M = sum |x w| + |b| plus the error so far:
    e = e_x |w| + 19 (2^-11 M (1 + 19 * 2^-11) + 2^-25); 2^-25 is half the subnormal spacing.
    Loose (no cancellation of the roundings is assumed) but it holds for every order."""
    v, e = x
    C = v.shape[1]
    w = wd_h.double().reshape(C, 1, 3, 3)
    b = bd_h.double()[None, :, None, None]
    conv = _conv(stride, dil, dil, C)
    out = conv(v.double(), w) + b
    mag = conv(v.double().abs() if e is None else v.double().abs() + e, w.abs()) + b.abs()
    err = 19.0 * (2.0 ** -11 * mag * (1.0 + 19 * 2.0 ** -11) + 2.0 ** -25)
    if e is not None:
        err = err + conv(e.double(), w.abs())
    return BR.act((out, err), act)


def unpack_fused_band(packed, stride, residual):
    """The operands of the band and slice kernels back out of ``fused_band.pack_fused_band``'s
    blob (the layout ``fused_band.emulate_fused_band`` reads), as a ``fused_ir_bound`` dict.
    ReLU6 is folded into [0, 1] clamps as in the stream kernel."""
    import numpy as np
    blob = packed["blob"].cpu().numpy()
    Cin, Cout, hidP = packed["Cin"], packed["Cout"], packed["hidP"]
    NSH, NCH, NS = hidP // 16, hidP // 32, -(-Cout // 16)
    fe = (blob[:NSH * 1024].view(np.uint16).astype(np.uint32) << 16).view(np.float32)
    We = fe.reshape(NSH, 4, 16, 8).transpose(0, 2, 1, 3).reshape(hidP, 32)
    be = blob[packed["o_be"]:packed["o_be"] + hidP * 4].view(np.float32)
    wd = blob[packed["o_wd"]:packed["o_wd"] + 18 * hidP].view(np.float16).reshape(9, hidP)
    bd = blob[packed["o_bd"]:packed["o_bd"] + 2 * hidP].view(np.float16)
    fp = blob[packed["o_wp"]:packed["o_wp"] + NS * NCH * 1024].view(np.float16)
    Wp = fp.reshape(NS, NCH, 4, 16, 8).transpose(0, 3, 1, 2, 4).reshape(NS * 16, hidP)
    bp = blob[packed["o_bp"]:packed["o_bp"] + NS * 64].view(np.float32)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a).copy())
    return dict(Cin=Cin, Cout=Cout, hidP=hidP, stride=stride, residual=residual, act="unit", chain="bias_last",
                we=t(We), be=t(be), wd_h=t(wd), bd_h=t(bd), wp_h=t(Wp), bp=t(bp))


def stem_pixels(frames, lut_x, lut_y, bf16):
    """The letterboxed, normalised model input (N, 3, H, W) as the stem kernels form it: one
    fused multiply-add per pixel (tests/int8_ref.py ``stem_pixel_table``), rounded to bf16 for
    the MFMA kernels. Exact: a table of 256 values."""
    import int8_ref as I
    import numpy as np
    x = I.letterbox_pixels(frames, torch.from_numpy(np.array(lut_x)), torch.from_numpy(np.array(lut_y)),
                           I.stem_pixel_table())
    return x.to(torch.bfloat16) if bf16 else x


def stem_bound(x, w, b, *, act, bf16_weights):
    """stem_conv (fp32 operands, per-lane) and stem_mfma (operands rounded to bf16): a k x k
    stride-2 conv of the normalised pixels, fp32 sum of 3 k k products + bias, the activation,
    one rounding to bf16."""
    w = w.to(torch.bfloat16) if bf16_weights else w
    return conv_bound(x, w, b, stride=2, act=act)


def stem_block0_bound(x, P):
    """stem_block0 and stem_band (fused_ir.hip, stem_band.hip; bit-identical to each other).
    ``P`` from ``pack_stem_block0``, x the bf16 pixels. Rounding points: the stem conv on bf16
    MFMA (weights / 6 in bf16, fp32 sum of 27 products + fp32 bias / 6), converted to fp16 and
    clamped to [0, 1] (ReLU6 / 6); the depthwise as the fp16 chain of ``dw_chain_fp16`` (bias / 6
    first, taps in raster order, [0, 1] clamp on the last fma); the projection on fp16 MFMA
    (weights x 6), fp32 sum of 32 products + fp32 bias, one rounding to bf16."""
    cpu = lambda t: t.detach().cpu()
    ws = cpu(P["ws"]).float().reshape(32, 12, 4)[:, :9, :3].reshape(32, 3, 3, 3).permute(0, 3, 1, 2)
    hid = conv_bound(x, ws, cpu(P["bs"]), stride=2, act="unit", fmt="fp16")
    d = dw_chain_fp16(hid, cpu(P["wd_h"]).t(), cpu(P["bd_h"]), stride=1, dil=1, act="unit")
    return conv_bound(d[0], cpu(P["wp_h"])[:, :, None, None], cpu(P["bp"]), x_err=d[1])


def unpack_fused_span(packed):
    """The operands of the stream kernel back out of ``fused_span.pack_fused_span``'s chunk
    images (the layout ``fused_span.emulate_fused_span`` reads), as a ``fused_ir_bound`` dict.
    ReLU6 is folded into [0, 1] clamps there: expansion weights and bias / 6 (bf16, fp32), the
    depthwise bias / 6 (fp16), the projection x 6 (fp16)."""
    import numpy as np
    Cin, Cout, hidP = packed["Cin"], packed["Cout"], packed["hidP"]
    KS, NS, NC = Cin // 32, Cout // 16, hidP // 32
    img = packed["w"].cpu().numpy().reshape(NC, -1)
    We, Wp, wd, bd, be = [], [], [], [], []
    for ch in img:
        fe = (ch[: 2 * KS * 1024].view(np.uint16).astype(np.uint32) << 16).view(np.float32)
        We.append(fe.reshape(2, KS, 4, 16, 8).transpose(0, 3, 1, 2, 4).reshape(32, Cin))
        fpj = ch[2 * KS * 1024:(2 * KS + NS) * 1024].view(np.float16).astype(np.float32)
        Wp.append(fpj.reshape(NS, 4, 16, 8).transpose(0, 2, 1, 3).reshape(Cout, 32))
        misc = ch[(2 * KS + NS) * 1024:]
        wd.append(misc[:576].view(np.float16).astype(np.float32).reshape(9, 32))
        bd.append(misc[576:640].view(np.float16).astype(np.float32))
        be.append(misc[640:768].view(np.float32).copy())
    t = lambda a, ax: torch.from_numpy(np.concatenate(a, ax).copy())
    return dict(Cin=Cin, Cout=Cout, hidP=hidP, stride=1, act="unit", we=t(We, 0), be=t(be, 0),
                wd_h=t(wd, 1).half(), bd_h=t(bd, 0).half(), wp_h=t(Wp, 1).half(), bp=packed["bp"].cpu())


def fused_ir_bound(x, P, *, tile):
    """An inverted-residual block in one kernel, from the operands ``pack_fused_ir`` packs
    (the quantised weights ARE the kernel's). x NCHW bf16.

    Row kernel (``tile`` False, fused_ir.hip ``fused_ir_kernel``): expansion on bf16 MFMA
    (fp32 sum of Cin products, + fp32 bias), ReLU6, rounded to bf16 into LDS; depthwise in fp32
    (fp32 weights, bias first, 9 taps), ReLU6, rounded to bf16 as the MFMA operand; projection
    on bf16 MFMA (fp32 sum of hid products) + fp32 bias + the bf16 input as residual, rounded to
    bf16. Without expansion the depthwise reads the input.

    Tile kernel (``tile`` True, ``fused_ir_tile_kernel``, fp16 internals): expansion as above
    but rounded to FP16 (the clamp after the conversion equals the conversion of the clamp: 0
    and 6 are fp16 numbers); without expansion the bf16 input is converted to fp16 (exact above
    2^-14); the depthwise is the fp16 chain of ``dw_chain_fp16`` on fp16 weights; the projection
    is an fp16 MFMA on fp16 weights with an fp32 accumulator, + fp32 bias + residual, rounded to
    bf16. The depthwise zero padding applies to the expanded tensor.

    The stream kernel (fused_ir_stream.hip, raster and lattice spans alike, ``P`` from
    ``unpack_fused_span``, ``act`` "unit") is the tile kernel's chain with ReLU6 folded into
    [0, 1] clamps; its hidden split adds fp32 partials of the same projection sum
    (``stream_combine`` or the in-launch combine), which the any-order bound covers.

    The band and slice kernels (fused_ir_band.hip, fused_ir_slice.hip; ``P`` from
    ``unpack_fused_band``, ``chain`` "bias_last") are the same chain with the depthwise bias
    added last (``dw_chain_fp16``). ``chain`` "loose" replaces the depthwise stage by the
    order-free bound without resets (``dw_fp16_loose``)."""
    cin, cout, s, dil, clamp = P["Cin"], P["Cout"], P["stride"], P.get("dil", 1), P.get("act", "relu6")
    cpu = lambda t: t.detach().cpu()
    # the zero-padded hidden channels (hidP) are kept: zero weights and biases, exact zeros
    hid = P["hidP"]
    if P["we"] is not None:
        pair = conv_bound(x, cpu(P["we"])[:, :cin, None, None], cpu(P["be"]), act=clamp,
                          fmt="fp16" if tile else "bf16")
    else:
        pair = (F.pad(x.double(), (0, 0, 0, 0, 0, hid - cin)), None)
        if tile:
            pair = BR.round_stage(pair[0], None, "fp16")
    if tile:
        wd, bd = cpu(P["wd_h"]).t()[:hid], cpu(P["bd_h"])[:hid]
        dw = dw_fp16_loose if P.get("chain") == "loose" else dw_chain_fp16
        d = dw(pair, wd, bd, stride=s, dil=dil, act=clamp, bias_last=P.get("chain") == "bias_last")
        wp = cpu(P["wp_h"])[:cout, :hid]
    else:
        wd, bd = cpu(P["wd"]).t()[:hid].reshape(hid, 1, 3, 3), cpu(P["bd"])[:hid]
        d = conv_bound(pair[0], wd, bd, stride=s, dil=dil, act="relu6", groups=hid, x_err=pair[1])
        wp = cpu(P["wp"])[:cout, :hid]
    res = x if P["residual"] else None
    return conv_bound(d[0], wp[:, :, None, None], cpu(P["bp"])[:cout], res=res, x_err=d[1])


def dw_proj_fused_bound(x, wd, bd, wp, bp, *, stride, dil, res=None):
    """dw_proj_fused (dw_proj.hip, fp16 internals; both the per-lane and the row-tile form).
    The hidden input arrives in fp16 (the bf16 test input converted: exact above 2^-14);
    ``pack_dw_proj`` rounds the depthwise weights, its bias and the projection weights to
    fp16; the depthwise is the fp16 chain of ``dw_chain_fp16`` (bias first, taps in raster
    order, one rounding per fma, [0, 6] clamp) and feeds an fp16 MFMA with an fp32 accumulator
    over hid terms; + fp32 bias + bf16 residual, one rounding to bf16."""
    C = x.shape[1]
    h = BR.round_stage(x.double(), None, "fp16")
    d = dw_chain_fp16(h, wd.float().to(torch.float16).reshape(C, 9), bd.float().to(torch.float16),
                      stride=stride, dil=dil)
    return conv_bound(d[0], wp.float().to(torch.float16)[:, :, None, None], bp, res=res, x_err=d[1])


def aspp_head_bound(cat, wp, bp, wl, bl, img_rows=None):
    """aspp_head (aspp_head.hip): proj = relu(Wp cat + bp + per-image bias), an fp32 sum of
    1024 products, rounded to bf16 into the on-chip projection tile; logits = Wl proj + bl, an
    fp32 sum of 256 products, rounded to bf16."""
    proj = mat_bound(cat, wp, bp, act="relu", img_rows=img_rows)
    return mat_bound(proj[0], wl, bl, x_err=proj[1])


ASPP_HEAD = [  # M, HW, ncls, ldo, img
    (32 * 33 * 33, 33 * 33, 21, 24, True),   # the B = 32 headline head (G = 9)
    (33 * 33, 33 * 33, 21, 24, True),        # batch 1 (G = 1)
    (4 * 33 * 33, 33 * 33, 19, 20, False),   # Cityscapes classes, no pooling branch
    (3 * 121 + 0, 121, 32, 32, True),        # M tail inside a 16-pixel group, full 32 classes
]
DW_PROJ_FUSED = DW_PROJECT + [(384, 64, 1, 1, True)]


def gen_aspp_head(M, HW, ncls, img):
    g = torch.Generator().manual_seed(11)
    cat = torch.relu(torch.randn(M, 1024, generator=g)).to(torch.bfloat16)
    wp = (torch.randn(256, 1024, generator=g) / 1024 ** 0.5).to(torch.bfloat16)
    bp = torch.randn(256, generator=g) * 0.1
    wl = (torch.randn(ncls, 256, generator=g) / 16).to(torch.bfloat16)
    bl = torch.randn(ncls, generator=g)
    ib = torch.randn(M // HW, 256, generator=g) * 0.5 if img else None
    return cat, wp, bp, wl, bl, ib


# ---------------------------------------------------------------- inputs of the CPU tier
def gen_conv(seed, B, H, W, Cin, Cout, k, stride=1, dil=1, res=False):
    """The draws of test_conv_gemm / _tap_grouped / test_tap_conv (same order)."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.randn(B, Cin, H, W, generator=g).to(torch.bfloat16)
    w = (torch.randn(Cout, Cin, k, k, generator=g) / (Cin * k * k) ** 0.5).to(torch.bfloat16)
    b = torch.randn(Cout, generator=g)
    pad = dil * (k // 2)
    OH = (H + 2 * pad - dil * (k - 1) - 1) // stride + 1
    OW = (W + 2 * pad - dil * (k - 1) - 1) // stride + 1
    r = torch.randn(B, Cout, OH, OW, generator=g).to(torch.bfloat16) if res else None
    return x, w, b, r


def gen_stem(cam, k, cout, H=129):
    """The draws of test_stem_fused_preprocess: (frames, lut_x, lut_y, w, b)."""
    import numpy as np
    from semantic_segmentation_server_amd.ops import reference_ops as R
    Wc, Hc = cam
    lx, ly, *_ = R.letterbox_luts(Wc, Hc, H, H)
    frames = torch.from_numpy(np.random.default_rng(4).integers(0, 256, (2, Hc, Wc, 3), dtype=np.uint8))
    g = torch.Generator().manual_seed(5)
    w = torch.randn(cout, 3, k, k, generator=g) / 4
    return frames, lx, ly, w, torch.randn(cout, generator=g)


def stem_block0_case(cam, H, frame_seed, device):
    """The stem + block 0 of test_stem_block0_fused / test_stem_band (BN folded, statistics
    from a seeded generator) with ``pack_stem_block0``'s operands on ``device``:
    (stem, blk, frames, lut_x, lut_y, P)."""
    from semantic_segmentation_server_amd.models.layers import ConvBNAct, init_random
    from semantic_segmentation_server_amd.models.mobilenetv2 import InvertedResidual, IRSpec
    from semantic_segmentation_server_amd.ops import hip_ops
    from semantic_segmentation_server_amd.ops import reference_ops as R
    stem = ConvBNAct(3, 32, 3, 2, act="relu6")
    blk = InvertedResidual(IRSpec(32, 16, 1, 1, 1))
    init_random(stem, seed=5)
    init_random(blk, seed=6)
    g = torch.Generator().manual_seed(56)
    for m in list(stem.modules()) + list(blk.modules()):
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_mean.uniform_(-0.2, 0.2, generator=g)
            m.running_var.uniform_(0.5, 2.0, generator=g)
    stem.eval()
    blk.eval()
    Wc, Hc = cam
    frames = torch.randint(0, 256, (2, Hc, Wc, 3), generator=torch.Generator().manual_seed(frame_seed),
                           dtype=torch.uint8)
    lx, ly, *_ = R.letterbox_luts(Wc, Hc, H, H)
    dwf, dbf = blk.dw.fold()
    pwf, pbf = blk.project.fold()
    P = hip_ops.pack_stem_block0(stem, dwf[:, 0], dbf, pwf[:, :, 0, 0], pbf, device)
    return stem, blk, frames, lx, ly, P


def stem_block0_emulate(x, P, order="whole"):
    """A correct stem + block 0 kernel: fp32 accumulators, roundings where ``stem_block0_bound``
    says (the block is ``fused_ir_emulate``'s tile chain without expansion on the fp16 stem
    output, [0, 1] clamps)."""
    cpu = lambda t: t.detach().cpu()
    ws = cpu(P["ws"]).float().reshape(32, 12, 4)[:, :9, :3].reshape(32, 3, 3, 3).permute(0, 3, 1, 2)
    h = conv_emulate(x, ws, cpu(P["bs"]), stride=2, act="unit", fmt="fp16", order=order)
    blk = dict(Cin=32, Cout=P["Cout"], hidP=32, stride=1, act="unit", we=None, residual=False,
               wd_h=cpu(P["wd_h"]), bd_h=cpu(P["bd_h"]), wp_h=cpu(P["wp_h"]), bp=cpu(P["bp"]))
    return fused_ir_emulate(h, blk, tile=True, order=order)


def ir_block(cin, cout, t, stride, dil, seed, device):
    """The random inverted-residual block of test_fused_inverted_residual / test_fused_ir_tile
    (BN folded) and its ``pack_fused_ir`` operands on ``device``."""
    from semantic_segmentation_server_amd.models.layers import init_random
    from semantic_segmentation_server_amd.models.mobilenetv2 import InvertedResidual, IRSpec
    from semantic_segmentation_server_amd.ops import hip_ops
    spec = IRSpec(cin, cout, t, stride, dil)
    blk = InvertedResidual(spec)
    init_random(blk, seed=seed)
    g = torch.Generator().manual_seed(seed)
    for m in blk.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_mean.uniform_(-0.2, 0.2, generator=g)
            m.running_var.uniform_(0.5, 2.0, generator=g)
    blk.eval()
    ew = eb = None
    if blk.expand is not None:
        ew, eb = blk.expand.fold()
        ew = ew[:, :, 0, 0]
    dwf, dbf = blk.dw.fold()
    pwf, pbf = blk.project.fold()
    packed = hip_ops.pack_fused_ir(ew, eb, dwf[:, 0], dbf, pwf[:, :, 0, 0], pbf, Cin=cin, hid=spec.hidden,
                                   Cout=cout, stride=stride, residual=spec.residual, device=device, dil=dil)
    return blk, packed


FUSED_IR = [  # cin, cout, t, stride, H  (test_fused_inverted_residual: W = H + 6, seed cin + cout)
    (32, 16, 1, 1, 37), (16, 24, 6, 2, 41), (24, 24, 6, 1, 33), (24, 32, 6, 2, 29), (32, 64, 6, 2, 21),
    (64, 64, 6, 1, 19), (64, 96, 6, 1, 17)]
FUSED_IR_STREAM = [  # cin, cout, dil, H, S  (W = 33)
    (64, 64, 1, 33, 8),     # blocks 7-9 (residual)
    (64, 96, 1, 33, 8),     # block 10
    (96, 96, 1, 33, 8),     # blocks 11-12 (residual)
    (96, 160, 1, 33, 8),    # block 13
    (160, 160, 2, 33, 8),   # blocks 14-15 (dilation 2, residual)
    (160, 160, 2, 33, 16),  # 16 spans per image
    (160, 320, 2, 33, 8),   # block 16 (3-slot ring, two epilogue passes)
    (64, 64, 1, 33, 32),    # batch-1 span counts
    (96, 96, 1, 29, 7),     # odd map height / span sizes
]
FUSED_IR_LATTICE = [  # cout, H, S  (cin 160, dilation 2, W = 33)
    (160, 33, 8),    # blocks 14-15 at the headline span count (residual)
    (160, 33, 16),   # batch-1 span counts
    (320, 33, 8),    # block 16 (two epilogue passes, group 8 on the expansion waves)
    (160, 21, 5),    # odd map height: classes of 11 / 10 rows, spans across class seams
]
STEM = [((640, 480), 3, 32), ((300, 411), 3, 32), ((640, 480), 7, 64)]  # cam, k, cout (H = W = 129)
STEM_BLOCK0 = [  # cam, H, tile  (test_stem_block0_fused; frames from seed 3)
    ((640, 480), 513, (8, 16)), ((200, 150), 129, (4, 16)), ((97, 131), 65, (8, 8)),
    ((640, 480), 129, (16, 16)), ((200, 150), 129, (8, 32)), ((97, 131), 65, (12, 16))]
STEM_BAND = [((640, 480), 513), ((160, 120), 129), ((200, 150), 97), ((96, 160), 129)]  # cam, H (seed 4)
STEM_BAND_MAX_H = 129  # test_stem_band bounds maps up to here; larger ones are bit-identical to stem_block0
# the (cam, H, frame seed) inputs whose stem + block 0 reference a device test uses
STEM_BLOCK0_INPUTS = sorted({(c, H, 3) for c, H, _ in STEM_BLOCK0} |
                            {(c, H, 4) for c, H in STEM_BAND if H <= STEM_BAND_MAX_H})
FUSED_IR_BAND = [  # cin, cout, stride, H, W  (test_fused_ir_band and test_fused_ir_slice)
    (16, 24, 2, 257, 257),   # block 1 (3 column bands, the last 1 column wide)
    (24, 24, 1, 129, 129),   # block 2 (residual)
    (24, 32, 2, 129, 129),   # block 3
    (32, 32, 1, 65, 65),     # blocks 4-5 (residual)
    (32, 64, 2, 65, 65),     # block 6
    (24, 24, 1, 100, 129),   # rows not a multiple of R
    (32, 32, 1, 7, 65),      # fewer rows than R
]
FUSED_IR_TILE = [  # cin, cout, stride, dil, H, tile  (W = H + 4, seed cin + 3 cout + dil)
    (64, 64, 1, 1, 33, (11, 11)),    # residual, CinP 64
    (64, 96, 1, 1, 33, (5, 11)),
    (96, 96, 1, 1, 33, (11, 11)),    # CinP 96
    (96, 160, 1, 1, 33, (11, 11)),
    (160, 160, 1, 2, 33, (11, 11)),  # dilation 2 + residual, CinP 160
    (160, 320, 1, 2, 33, (5, 11)),   # Cout 320
    (160, 160, 1, 2, 29, (8, 16)),   # partial tiles at the right/bottom edge
    (24, 32, 2, 1, 65, (8, 16)),     # stride 2, CinP 32
    (32, 64, 2, 1, 65, (5, 11)),
    (16, 24, 2, 1, 67, (5, 11)),     # block 1 shape (CinP 32 from Cin 16)
    (24, 24, 1, 1, 41, (11, 11)),    # block 2 shape: residual, Cin 24 -> CinP 32
    (32, 32, 1, 1, 30, (8, 13)),     # blocks 4/5, partial edge tiles
    (32, 16, 1, 1, 37, (8, 16)),     # block 0: no expansion (t = 1)
]


# ---------------------------------------------------------------- fp32 emulations (CPU tier)
def fused_ir_emulate(x, P, *, tile, order="whole", hidden_hook=None, res=None):
    """A correct fused block: fp32 accumulators, roundings where ``fused_ir_bound`` says.
    ``res``: a residual other than the block's input (dw_proj_fused)."""
    cin, cout, s, dil, hid = P["Cin"], P["Cout"], P["stride"], P.get("dil", 1), P["hidP"]
    fmt = "fp16" if tile else "bf16"
    clamp = P.get("act", "relu6")
    if P["we"] is not None:
        h = conv_emulate(x, P["we"][:, :cin, None, None], P["be"], act=clamp, fmt=fmt, order=order)
    else:
        h = F.pad(x, (0, 0, 0, 0, 0, hid - cin)).to(BR.TORCH_DTYPE[fmt])
    if tile:
        w = P["wd_h"].t().double()
        bias = P["bd_h"].double()[None, :, None, None]
        last = P.get("chain") in ("loose", "bias_last")  # band / slice: from zero, bias last
        d = torch.zeros(()) if last else bias
        for t, hv in enumerate(_tap_views(h.double(), 3, s, dil)):
            # the exact sum, rounded ONCE as the fma does (torch casts float64 through fp32: twice)
            d = BR.rnd(d + hv * w[:, t][None, :, None, None], "fp16")
        if last:
            d = BR.rnd(d + bias, "fp16")
        d = d.clamp(0.0, 6.0 if clamp == "relu6" else 1.0).half()
        wp = P["wp_h"][:cout]
    else:
        d = conv_emulate(h, P["wd"].t().reshape(hid, 1, 3, 3), P["bd"], stride=s, dil=dil, act="relu6",
                         groups=hid, order=order)
        wp = P["wp"][:cout]
    if hidden_hook is not None:
        d = hidden_hook(d)
    res = x if res is None and P["residual"] else res
    return conv_emulate(d, wp[:, :, None, None], P["bp"][:cout], res=res, order=order)



def sum_taps(xf, wf, stride, dil, groups=1, skip=None):
    """fp32 sum of the per-tap partial convs (each a 1 x 1 conv of a shifted view of the padded
    input), in tap order; ``skip`` = (i, j) leaves that tap out."""
    k = wf.shape[-1]
    pad = dil * (k // 2)
    H, W = xf.shape[-2:]
    OH = (H + 2 * pad - dil * (k - 1) - 1) // stride + 1
    OW = (W + 2 * pad - dil * (k - 1) - 1) // stride + 1
    xp = F.pad(xf, (pad, pad, pad, pad))
    acc = None
    for i in range(k):
        for j in range(k):
            if (i, j) == skip:
                continue
            xs = xp[:, :, i * dil:i * dil + (OH - 1) * stride + 1:stride,
                    j * dil:j * dil + (OW - 1) * stride + 1:stride]
            part = F.conv2d(xs, wf[:, :, i:i + 1, j:j + 1], None, 1, 0, 1, groups)
            acc = part if acc is None else acc + part
    return acc


def mat_emulate(x, w, b, *, act=None, res=None, img_rows=None, fmt="bf16", order="whole"):
    xf, wf = x.float(), w.float()
    if order == "whole":
        acc = xf @ wf.t()
    else:
        step = -(-x.shape[1] // 4)
        acc = None
        for c in range(0, x.shape[1], step):
            part = xf[:, c:c + step] @ wf[:, c:c + step].t()
            acc = part if acc is None else acc + part
    for t in (None if b is None else b.float()[None, :], img_rows, res):
        if t is not None:
            acc = acc + t.float()
    acc = BR.act((acc, None), act)[0]
    return acc.to(BR.TORCH_DTYPE[fmt]) if fmt else acc


def conv_emulate(x, w, b, *, stride=1, dil=1, act=None, res=None, img_bias=None, groups=1, fmt="bf16",
                 order="whole"):
    """What a kernel with fp32 accumulators computes. ``whole``: one fp32 conv; ``parts``: the
    sum of per-tap partial convs (k > 1) or of four Cin-chunk partial convs (k = 1), as a
    tap loop or a split-K kernel adds them."""
    k = w.shape[-1]
    xf, wf = x.float(), w.float()
    pad = dil * (k // 2)
    if order == "whole":
        acc = F.conv2d(xf, wf, None, stride, pad, dil, groups)
    elif k > 1:
        acc = sum_taps(xf, wf, stride, dil, groups)
    else:
        assert groups == 1
        acc = None
        step = -(-x.shape[1] // 4)
        for c in range(0, x.shape[1], step):
            part = F.conv2d(xf[:, c:c + step], wf[:, c:c + step], None, stride)
            acc = part if acc is None else acc + part
    acc = acc + b.float()[None, :, None, None]
    if img_bias is not None:
        acc = acc + img_bias.float()[:, :, None, None]
    if res is not None:
        acc = acc + res.float()
    acc = BR.act((acc, None), act)[0]
    return acc.to(BR.TORCH_DTYPE[fmt]) if fmt else acc
