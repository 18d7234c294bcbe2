"""T3 kernel goldens: every gfx950 kernel vs a plain PyTorch fp32 reference.

Data is random and asymmetric (a transposed C-write cannot pass), shapes cover
the model's channel counts, strides and dilations. bf16 tolerances: inputs are
bf16-rounded for both sides, so the only differences are accumulation order and
the final bf16 rounding of the output.

Beside every norm check of a bf16 / fp16 kernel stands an elementwise one (``_within``):
``|got - v| <= e`` at every element, v a float64 reference that rounds where the kernel rounds
and e its derived bound (tests/bound_ref.py, tests/bound_cases.py; the bound itself is judged
on the CPU in tests/test_bound_ref_cpu.py). A norm hides a handful of wrong elements; this
does not. The outputs of the conv, GEMM, depthwise (+ projection), row / tile fused-block and head kernels
(every writer into a channel slice among them) sit between guard rows that must come back
untouched; the stem, stream, band and slice kernels write plain NaN-filled buffers.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bound_cases as BC
import bound_ref as BR
import upsample_ref as UR

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _hip():
    from semantic_segmentation_server_amd.ops import hip_ops
    return hip_ops


def _rel(a, b):
    a, b = a.float(), b.float()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


_BOUND = {}
GUARD_ROWS = 8  # whole rows of the fill value before and after an output buffer


def _bound(key, make):
    """The float64 reference pair (v, e) of a shape (tests/bound_ref.py), computed once and
    shared by every variant of that shape."""
    if key not in _BOUND:
        _BOUND[key] = make()
    return _BOUND[key]


def _within(got, ref, what):
    """|got - v| <= e at every element, beside the norm check of the same output."""
    ratio = BR.assert_within(got, ref[0], ref[1], what)
    print(f"[bound] {what}: max |got - v| / e = {ratio:.3f}, flip possible at {BR.flip_share(ref[1]):.3e}")
    return ratio


def _guarded_out(shape, fill, dtype=torch.bfloat16):
    """An output of ``shape`` = (..., ldo) inside a buffer with GUARD_ROWS rows of ``fill``
    before and after it: (buffer, view)."""
    M = int(np.prod(shape[:-1]))
    raw = torch.full((M + 2 * GUARD_ROWS, shape[-1]), fill, dtype=dtype, device=DEV)
    return raw, raw[GUARD_ROWS:GUARD_ROWS + M].view(shape)


def _guards_kept(raw, fill):
    """Nothing was written before the first or past the last row of the output."""
    g = torch.cat([raw[:GUARD_ROWS], raw[-GUARD_ROWS:]]).float()
    return bool(torch.all(g == fill)) if fill == fill else bool(torch.isnan(g).all())


def _nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def _nchw(x):
    return x.permute(0, 3, 1, 2).contiguous()


@pytest.mark.parametrize("B,H,W,Cin,Cout,k,stride,dil,act,res,ldo_pad,co_off", BC.CONV_GEMM)
@pytest.mark.parametrize("variant", [1, 2, 3, 4, 5, 6, 7])
def test_conv_gemm(B, H, W, Cin, Cout, k, stride, dil, act, res, ldo_pad, co_off, variant):
    K = _hip()
    g = torch.Generator(device="cpu").manual_seed(1)
    x = torch.randn(B, Cin, H, W, generator=g).to(torch.bfloat16)
    w = (torch.randn(Cout, Cin, k, k, generator=g) / (Cin * k * k) ** 0.5).to(torch.bfloat16)
    b = torch.randn(Cout, generator=g)
    ref = F.conv2d(x.float(), w.float(), b, stride, dil * (k // 2), dil)
    OH, OW = ref.shape[-2:]
    r = None
    if res:
        r = torch.randn(B, Cout, OH, OW, generator=g).to(torch.bfloat16)
        ref = ref + r.float()
    if act == "relu":
        ref = F.relu(ref)
    elif act == "relu6":
        ref = F.relu6(ref)
    ldo = co_off + Cout + ldo_pad
    raw, out = _guarded_out((B, OH, OW, ldo), 7.0)
    K.conv_gemm(_nhwc(x).to(DEV), w.permute(0, 2, 3, 1).contiguous().to(DEV), b.to(DEV), out,
                B=B, IH=H, IW=W, Cin=Cin, OH=OH, OW=OW, Cout=Cout, k=k, stride=stride, dil=dil,
                ldo=ldo, co_off=co_off, act=act,
                res=None if r is None else _nhwc(r).to(DEV), variant=variant)
    torch.cuda.synchronize()
    got = out[..., co_off:co_off + Cout]
    assert _rel(_nchw(got).cpu(), ref) < 1e-2
    bound = _bound(("conv_gemm", B, H, W, Cin, Cout, k, stride, dil, act, res),
                   lambda: BC.conv_bound(x, w, b, stride=stride, dil=dil, act=act, res=r))
    _within(_nchw(got), bound, f"conv_gemm variant {variant}")
    assert _guards_kept(raw, 7.0)
    # untouched channels keep their sentinel
    if co_off:
        assert torch.all(out[..., :co_off] == 7.0)
    if ldo_pad:
        assert torch.all(out[..., co_off + Cout:] == 7.0)


@pytest.mark.parametrize("B,H,W,rate", BC.TAP_GROUPED)
@pytest.mark.parametrize("variant,bm", [(3, 128), (4, 128), (5, 128), (6, 256)])
def test_conv_gemm_tap_grouped(B, H, W, rate, variant, bm):
    """Dilated 3x3 through the tap-validity permutation: same result as raster order,
    channel-slice write, padding rows (-1) write nothing."""
    K = _hip()
    Cin, Cout, co_off, ldo = 64, 96, 32, 160
    g = torch.Generator().manual_seed(5)
    x = torch.randn(B, Cin, H, W, generator=g).to(torch.bfloat16)
    w = (torch.randn(Cout, Cin, 3, 3, generator=g) / (Cin * 9) ** 0.5).to(torch.bfloat16)
    b = torch.randn(Cout, generator=g)
    ref = F.relu(F.conv2d(x.float(), w.float(), b, 1, rate, rate))
    perm = K.tap_group_perm(B, H, W, 3, rate, bm, DEV)
    assert perm.numel() % bm == 0
    raw, out = _guarded_out((B, H, W, ldo), 7.0)
    K.conv_gemm(_nhwc(x).to(DEV), w.permute(0, 2, 3, 1).contiguous().to(DEV), b.to(DEV), out,
                B=B, IH=H, IW=W, Cin=Cin, OH=H, OW=W, Cout=Cout, k=3, dil=rate, ldo=ldo,
                co_off=co_off, act="relu", variant=variant, perm=perm)
    torch.cuda.synchronize()
    assert _rel(_nchw(out[..., co_off:co_off + Cout]).cpu(), ref) < 1e-2
    bound = _bound(("tap_grouped", B, H, W, rate), lambda: BC.conv_bound(x, w, b, dil=rate, act="relu"))
    _within(_nchw(out[..., co_off:co_off + Cout]), bound, f"conv_gemm tap-grouped variant {variant}")
    assert _guards_kept(raw, 7.0)  # a padding row (perm -1) lands nowhere, not before the buffer
    assert torch.all(out[..., :co_off] == 7.0) and torch.all(out[..., co_off + Cout:] == 7.0)


@pytest.mark.parametrize("B,H,W,Cin,Cout,variant", BC.GROUPED_ASPP)
def test_conv_gemm_grouped_aspp(B, H, W, Cin, Cout, variant):
    """ASPP branches (1x1 + atrous 6/12/18, tap-grouped rows) in one LPT-ordered grid:
    each branch's channel slice matches F.conv2d, the other channels stay untouched."""
    K = _hip()
    g = torch.Generator().manual_seed(11)
    x = torch.randn(B, Cin, H, W, generator=g).to(torch.bfloat16)
    xd = _nhwc(x).to(DEV)
    ldo = 4 * Cout + 16
    raw, out = _guarded_out((B, H, W, ldo), 7.0)
    BM = K.GROUP_TILE[variant][0]
    convs, refs, bounds = [], [], []
    for j, (k, rate) in enumerate(BC.ASPP_BRANCHES):
        w = (torch.randn(Cout, Cin, k, k, generator=g) / (Cin * k * k) ** 0.5).to(torch.bfloat16)
        b = torch.randn(Cout, generator=g)
        refs.append(F.relu(F.conv2d(x.float(), w.float(), b, 1, rate * (k // 2), rate)))
        bounds.append(_bound(("grouped_aspp", B, H, W, Cin, Cout, j),
                             lambda: BC.conv_bound(x, w, b, dil=rate, act="relu")))
        convs.append(dict(x=xd, w=w.permute(0, 2, 3, 1).contiguous().to(DEV), bias=b.to(DEV), out=out,
                          B=B, IH=H, IW=W, Cin=Cin, OH=H, OW=W, Cout=Cout, k=k, dil=rate, ldo=ldo,
                          co_off=j * Cout, act="relu",
                          perm=K.tap_group_perm(B, H, W, 3, rate, BM, DEV) if k == 3 else None))
    order = K.grouped_tile_order(convs, variant, DEV)
    K.conv_gemm_grouped(convs, order, variant)
    torch.cuda.synchronize()
    for j, ref in enumerate(refs):
        assert _rel(_nchw(out[..., j * Cout:(j + 1) * Cout]).cpu(), ref) < 1e-2, j
        _within(_nchw(out[..., j * Cout:(j + 1) * Cout]), bounds[j], f"grouped ASPP variant {variant} branch {j}")
    assert torch.all(out[..., 4 * Cout:] == 7.0)
    assert _guards_kept(raw, 7.0)


@pytest.mark.parametrize("B,variant,ks", BC.GROUPED_SPLITK)
def test_conv_gemm_grouped_aspp_splitk(B, variant, ks):
    """Split-K grouped ASPP (batch-1 plans): the K slices' fp32 partials + stream_combine
    (bias, ReLU) vs F.conv2d per branch, bit-identical on a rerun, uneven stage splits
    (a 1x1 branch of 5 stages over 6 slices: empty slices write zeros)."""
    K = _hip()
    g = torch.Generator().manual_seed(12)
    H = W = 33
    Cin, Cout = 320, 256
    x = torch.randn(B, Cin, H, W, generator=g).to(torch.bfloat16)
    xd = _nhwc(x).to(DEV)
    ldo = 4 * Cout
    raw, out = _guarded_out((B, H, W, ldo), float("nan"))
    BM = K.GROUP_TILE[variant][0]
    convs, refs, biases, bounds = [], [], [], []
    for j, (k, rate) in enumerate(BC.ASPP_BRANCHES):
        w = (torch.randn(Cout, Cin, k, k, generator=g) / (Cin * k * k) ** 0.5).to(torch.bfloat16)
        b = torch.randn(Cout, generator=g)
        biases.append(b)
        refs.append(F.relu(F.conv2d(x.float(), w.float(), b, 1, rate * (k // 2), rate)))
        # n is the full K: the slices' fp32 partials are one fp32 sum in another order
        bounds.append(_bound(("grouped_splitk", B, j), lambda: BC.conv_bound(x, w, b, dil=rate, act="relu")))
        convs.append(dict(x=xd, w=w.permute(0, 2, 3, 1).contiguous().to(DEV), bias=b.to(DEV), out=out,
                          B=B, IH=H, IW=W, Cin=Cin, OH=H, OW=W, Cout=Cout, k=k, dil=rate, ldo=ldo,
                          co_off=j * Cout, act="relu",
                          perm=K.tap_group_perm(B, H, W, 3, rate, BM, DEV) if k == 3 else None))
    order = K.grouped_tile_order(convs, variant, DEV, ks=ks)
    part = torch.full((ks * B * H * W * ldo,), float("nan"), dtype=torch.float32, device=DEV)
    bias_cat = torch.cat(biases).to(DEV)
    K.conv_gemm_grouped(convs, order, variant, ks=ks, part=part, bias_cat=bias_cat)
    torch.cuda.synchronize()
    for j, ref in enumerate(refs):
        assert _rel(_nchw(out[..., j * Cout:(j + 1) * Cout]).cpu(), ref) < 1e-2, j
        _within(_nchw(out[..., j * Cout:(j + 1) * Cout]), bounds[j],
                f"split-K grouped ASPP variant {variant} ks {ks} branch {j}")
    assert _guards_kept(raw, float("nan"))
    first = out.clone()
    out.fill_(float("nan"))
    K.conv_gemm_grouped(convs, order, variant, ks=ks, part=part, bias_cat=bias_cat)
    torch.cuda.synchronize()
    assert torch.equal(first.view(torch.int16), out.view(torch.int16))
    # in-launch combine by each tile's last arriving K slice: same fixed-order sums, so
    # bit-identical to the combine kernel; tickets reset for the next launch
    cnt = torch.zeros(4 * 1024, dtype=torch.int32, device=DEV)
    for rep in range(3):
        out.fill_(float("nan"))
        K.conv_gemm_grouped(convs, order, variant, ks=ks, part=part, bias_cat=bias_cat, cnt=cnt)
        torch.cuda.synchronize()
        assert torch.equal(first.view(torch.int16), out.view(torch.int16)), rep
        assert int(cnt.abs().sum()) == 0, rep
    assert _guards_kept(raw, float("nan"))


@pytest.mark.parametrize("img", [True, False])
def test_bias_act(img):
    """GEMM epilogue: act(x + bias + per-image bias) vs torch."""
    K = _hip()
    g = torch.Generator().manual_seed(3)
    B, HW, N = 3, 37, 264
    x = torch.randn(B * HW, N, generator=g).to(torch.bfloat16)
    b = torch.randn(N, generator=g)
    ib = torch.randn(B, N, generator=g)
    ref = x.float() + b + (ib.repeat_interleave(HW, 0) if img else 0)
    ref = torch.relu(ref)
    raw, out = _guarded_out((B * HW, N), 7.0)
    K.bias_act(x.to(DEV), b.to(DEV), out, M=B * HW, N=N, HW=HW, img_bias=ib.to(DEV) if img else None,
               act="relu")
    torch.cuda.synchronize()
    assert _rel(out.float().cpu(), ref) < 1e-2
    _within(out, BC.bias_act_bound(x, b, ib.repeat_interleave(HW, 0) if img else None, "relu"), "bias_act")
    assert _guards_kept(raw, 7.0)


@pytest.mark.parametrize("B,H,W,Cin,Cout,rate,grouped", BC.TAP_CONV)
def test_tap_conv(B, H, W, Cin, Cout, rate, grouped):
    """tap_conv vs F.conv2d: raster or tap-grouped rows, channel-slice write, partial
    128-channel group (Cout % 128 != 0)."""
    K = _hip()
    co_off, extra = 8, 16
    ldo = co_off + Cout + extra
    g = torch.Generator().manual_seed(6)
    x = torch.randn(B, Cin, H, W, generator=g).to(torch.bfloat16)
    w = (torch.randn(Cout, Cin, 3, 3, generator=g) / (Cin * 9) ** 0.5).to(torch.bfloat16)
    b = torch.randn(Cout, generator=g)
    ref = F.relu(F.conv2d(x.float(), w.float(), b, 1, rate, rate))
    wpk, bp = K.pack_tap_weights(w.permute(0, 2, 3, 1).contiguous().to(DEV), b.to(DEV))
    perm = K.tap_group_perm(B, H, W, 3, rate, 256, DEV) if grouped else None
    raw, out = _guarded_out((B, H, W, ldo), 7.0)
    K.tap_conv(_nhwc(x).to(DEV), wpk, bp, out, B=B, H=H, W=W, Cin=Cin, Cout=Cout, k=3, dil=rate,
               ldo=ldo, co_off=co_off, act="relu", perm=perm)
    torch.cuda.synchronize()
    assert _rel(_nchw(out[..., co_off:co_off + Cout]).cpu(), ref) < 1e-2
    bound = _bound(("tap_conv", B, H, W, Cin, Cout, rate), lambda: BC.conv_bound(x, w, b, dil=rate, act="relu"))
    _within(_nchw(out[..., co_off:co_off + Cout]), bound, "tap_conv")
    assert _guards_kept(raw, 7.0)
    assert torch.all(out[..., :co_off] == 7.0) and torch.all(out[..., co_off + Cout:] == 7.0)


def test_conv_gemm_img_bias():
    K = _hip()
    B, H, W, Cin, Cout = 3, 5, 7, 64, 48
    g = torch.Generator().manual_seed(2)
    x = torch.randn(B, Cin, H, W, generator=g).to(torch.bfloat16)
    w = (torch.randn(Cout, Cin, 1, 1, generator=g) / 8).to(torch.bfloat16)
    b = torch.randn(Cout, generator=g)
    ib = torch.randn(B, Cout, generator=g)
    ref = F.relu(F.conv2d(x.float(), w.float(), b) + ib[:, :, None, None])
    raw, out = _guarded_out((B, H, W, Cout), 7.0)
    K.conv_gemm(_nhwc(x).to(DEV), w.permute(0, 2, 3, 1).contiguous().to(DEV), b.to(DEV), out, B=B,
                IH=H, IW=W, Cin=Cin, OH=H, OW=W, Cout=Cout, act="relu", img_bias=ib.to(DEV))
    torch.cuda.synchronize()
    assert _rel(_nchw(out).cpu(), ref) < 1e-2
    _within(_nchw(out), BC.conv_bound(x, w, b, act="relu", img_bias=ib), "conv_gemm img_bias")
    assert _guards_kept(raw, 7.0)


@pytest.mark.parametrize("M,Cin,Cout,act,res,img,ldo_pad,co_off,n_out", BC.PW_CONV)
@pytest.mark.parametrize("mt,nch", [(2, 1), (2, 3), (4, 2)])
def test_pw_conv(M, Cin, Cout, act, res, img, ldo_pad, co_off, n_out, mt, nch):
    K = _hip()
    g = torch.Generator().manual_seed(3)
    x = (torch.randn(M, Cin, generator=g) * 0.5).to(torch.bfloat16)
    w = (torch.randn(Cout, Cin, generator=g) / Cin ** 0.5).to(torch.bfloat16)
    b = torch.randn(Cout, generator=g)
    ref = x.float() @ w.float().t() + b
    N = n_out or Cout
    r = ib = None
    HW = 121 if img else 1
    if res:
        r = torch.randn(M, N, generator=g).to(torch.bfloat16)
        ref = ref + r.float()[:, :Cout]
    if img:
        ib = torch.randn(M // HW, N, generator=g)
        ref = ref + ib.repeat_interleave(HW, 0)[:, :Cout]
    if act == "relu":
        ref = F.relu(ref)
    elif act == "relu6":
        ref = F.relu6(ref)
    ldo = co_off + N + ldo_pad
    raw, out = _guarded_out((M, ldo), 7.0)  # rows past M: the last M tile is partial
    wpk = K.pack_pw_weights(w.to(DEV), b.to(DEV), N_out=N)
    K.pw_conv(x.to(DEV), wpk, out, M=M, K=Cin, N=N, ldo=ldo, co_off=co_off, act=act,
              res=None if r is None else r.to(DEV), img_bias=None if ib is None else ib.to(DEV),
              HW=HW, mt=mt, nch=nch)
    torch.cuda.synchronize()
    got = out[:, co_off:co_off + Cout].float().cpu()
    assert _rel(got, ref) < 1e-2
    bound = _bound(("pw_conv", M, Cin, Cout, act, res, img), lambda: BC.mat_bound(
        x, w, b, act=act, res=None if r is None else r[:, :Cout],
        img_rows=None if ib is None else ib.repeat_interleave(HW, 0)[:, :Cout]))
    _within(got, bound, f"pw_conv mt {mt} nch {nch}")
    assert _guards_kept(raw, 7.0)
    if N > Cout and not res and not img:  # padded channels: zero weights and bias -> act(0)
        assert torch.all(out[:, co_off + Cout:co_off + N].float() == 0)
    if co_off:
        assert torch.all(out[:, :co_off] == 7.0)
    if ldo_pad:
        assert torch.all(out[:, co_off + N:] == 7.0)


@pytest.mark.parametrize("B,H,W,C,stride,dil", BC.DEPTHWISE)
def test_depthwise(B, H, W, C, stride, dil):
    K = _hip()
    g = torch.Generator().manual_seed(3)
    x = torch.randn(B, C, H, W, generator=g).to(torch.bfloat16)
    w = torch.randn(C, 1, 3, 3, generator=g) / 3
    b = torch.randn(C, generator=g)
    ref = F.relu6(F.conv2d(x.float(), w, b, stride, dil, dil, groups=C))
    OH, OW = ref.shape[-2:]
    raw, out = _guarded_out((B, OH, OW, C), 7.0)
    K.depthwise3x3(_nhwc(x).to(DEV), w.reshape(C, 9).t().contiguous().to(DEV), b.to(DEV), out, B=B,
                   IH=H, IW=W, C=C, OH=OH, OW=OW, stride=stride, dil=dil, act="relu6")
    torch.cuda.synchronize()
    assert _rel(_nchw(out).cpu(), ref) < 1e-2
    bound = _bound(("depthwise", B, H, W, C, stride, dil),
                   lambda: BC.conv_bound(x, w, b, stride=stride, dil=dil, act="relu6", groups=C))
    _within(_nchw(out), bound, "depthwise3x3")
    assert _guards_kept(raw, 7.0)


@pytest.mark.parametrize("cam,k,cout", BC.STEM)
def test_stem_fused_preprocess(cam, k, cout):
    from semantic_segmentation_server_amd.ops import reference_ops as R
    K = _hip()
    Wc, Hc = cam
    H = W = 129
    lx, ly, *_ = R.letterbox_luts(Wc, Hc, W, H)
    rng = np.random.default_rng(4)
    frames = torch.from_numpy(rng.integers(0, 256, (2, Hc, Wc, 3), dtype=np.uint8))
    x = R.preprocess(frames, lx, ly)  # fp32 NCHW
    g = torch.Generator().manual_seed(5)
    w = torch.randn(cout, 3, k, k, generator=g) / 4
    b = torch.randn(cout, generator=g)
    ref = F.relu6(F.conv2d(x, w, b, 2, k // 2))
    OH, OW = ref.shape[-2:]
    out = torch.empty(2, OH, OW, cout, dtype=torch.bfloat16, device=DEV)
    wk = w.permute(2, 3, 1, 0).reshape(-1, cout).contiguous().to(DEV)
    K.stem_conv(frames.to(DEV), torch.tensor(lx, device=DEV), torch.tensor(ly, device=DEV),
                wk, b.to(DEV), out, H=H, W=W, OH=OH, OW=OW, Cout=cout, k=k, stride=2, act="relu6")
    torch.cuda.synchronize()
    assert _rel(_nchw(out).cpu(), ref) < 1e-2
    _within(_nchw(out), BC.stem_bound(BC.stem_pixels(frames, lx, ly, False), w, b, act="relu6", bf16_weights=False),
            "stem_conv")
    mfma_bound = BC.stem_bound(BC.stem_pixels(frames, lx, ly, True), w, b, act="relu6", bf16_weights=True)
    # MFMA stem (bf16 operands): same conv, several tile shapes, bf16 and int8 outputs
    wpk = K.pack_stem_mfma(wk, k, cout)
    # (per_wave: one wave per 16 output channels, 7x7 / 64 channels only, tiles to 32 x 32)
    tiles = [((8, 16), False), ((16, 16), False), ((3, 7), False)]
    if (k, cout) == (7, 64):
        tiles += [((16, 16), True), ((16, 32), True), ((32, 32), True), ((5, 9), True)]
    for tile, pw in tiles:
        o2 = torch.full((2, OH, OW, cout), float("nan"), dtype=torch.bfloat16, device=DEV)
        K.stem_mfma(frames.to(DEV), torch.tensor(lx, device=DEV), torch.tensor(ly, device=DEV), wpk,
                    b.to(DEV), o2, H=H, W=W, OH=OH, OW=OW, Cout=cout, k=k, stride=2, act="relu6",
                    tile=tile, per_wave=pw)
        torch.cuda.synchronize()
        assert torch.isfinite(o2.float()).all()
        assert _rel(_nchw(o2).cpu(), ref) < 2e-2, tile
        _within(_nchw(o2), mfma_bound, f"stem_mfma tile {tile} per_wave {pw}")
    # int8 output against the conv of bf16-rounded operands in float64 (pixels normalised with
    # one rounding, as the kernels' fused multiply-add does): at most one step off, <= 1e-3
    import int8_ref as I
    xk = I.letterbox_pixels(frames, torch.tensor(lx.tolist()), torch.tensor(ly.tolist()), I.stem_pixel_table())
    exp = I.requant(torch.clamp(I.stem_ref_values(xk, w, b, 2, bf16_operands=True), 0.0, 6.0), 0.05)
    for tile, pw in [((8, 16), False)] + ([((32, 32), True)] if (k, cout) == (7, 64) else []):
        o8 = torch.empty(2, OH, OW, cout, dtype=torch.int8, device=DEV)
        K.stem_mfma(frames.to(DEV), torch.tensor(lx, device=DEV), torch.tensor(ly, device=DEV), wpk,
                    b.to(DEV), o8, H=H, W=W, OH=OH, OW=OW, Cout=cout, k=k, stride=2, act="relu6",
                    out_scale=0.05, tile=tile, per_wave=pw)
        torch.cuda.synchronize()
        I.assert_codes_close(_nchw(o8).cpu(), exp, f"stem_mfma int8 tile {tile}")
    if (k, cout) == (7, 64):
        # relu + int8 (the config-4 stem): the per-wave kernel's med3 + v_cvt_pk_u8 epilogue
        # gives the same codes as the all-blocks kernel's float chain (same MFMA sums)
        outs = []
        for tile, pw in (((8, 16), False), ((32, 32), True)):
            o8 = torch.full((2, OH, OW, cout), 99, dtype=torch.int8, device=DEV)
            K.stem_mfma(frames.to(DEV), torch.tensor(lx, device=DEV), torch.tensor(ly, device=DEV), wpk,
                        b.to(DEV), o8, H=H, W=W, OH=OH, OW=OW, Cout=cout, k=k, stride=2, act="relu",
                        out_scale=0.05, tile=tile, per_wave=pw)
            outs.append(o8)
        torch.cuda.synchronize()
        assert torch.equal(outs[0].cpu(), outs[1].cpu())
        assert int(outs[1].min()) >= 0


def test_maxpool_gap_matvec():
    K = _hip()
    g = torch.Generator().manual_seed(6)
    x = torch.randn(2, 64, 31, 29, generator=g).to(torch.bfloat16)
    ref = F.max_pool2d(x.float(), 3, 2, 1)
    OH, OW = ref.shape[-2:]
    out = torch.empty(2, OH, OW, 64, dtype=torch.bfloat16, device=DEV)
    K.maxpool3x3s2(_nhwc(x).to(DEV), out, B=2, IH=31, IW=29, C=64, OH=OH, OW=OW)
    gap = torch.empty(2, 64, device=DEV)
    K.global_avgpool(_nhwc(x).to(DEV), gap, B=2, HW=31 * 29, C=64)
    wm = torch.randn(40, 64, generator=g)
    bm = torch.randn(40, generator=g)
    mv = torch.empty(2, 40, device=DEV)
    K.matvec(gap, wm.to(DEV), bm.to(DEV), mv, B=2, N=40, K=64, act="relu")
    torch.cuda.synchronize()
    assert torch.equal(_nchw(out).cpu().float(), ref)
    gref = x.float().mean((2, 3))
    assert torch.allclose(gap.cpu(), gref, atol=1e-4)
    assert torch.allclose(mv.cpu(), F.relu(gref @ wm.t() + bm), atol=1e-3)
    gap_ref = BC.gap_bound(x)  # fp32 outputs: no rounding stage
    _within(gap, gap_ref, "global_avgpool")
    _within(mv, BC.mat_bound(gap_ref[0], wm, bm, act="relu", fmt=None, x_err=gap_ref[1]), "matvec of the GAP")


@pytest.mark.parametrize("B,N,K,bias", BC.MATVEC)
def test_matvec(B, N, K, bias):
    """fp32 matvec head (one wave per (b, n), lanes split K) against torch."""
    K_ = _hip()
    g = torch.Generator().manual_seed(N)
    x = torch.randn(B, K, generator=g)
    w = torch.randn(N, K, generator=g)
    b = torch.randn(N, generator=g) if bias else None
    out = torch.empty(B, N, device=DEV)
    K_.matvec(x.to(DEV), w.to(DEV), None if b is None else b.to(DEV), out, B=B, N=N, K=K, act="relu")
    torch.cuda.synchronize()
    ref = F.relu(x.double() @ w.double().t() + (0 if b is None else b.double()))
    assert torch.allclose(out.cpu().double(), ref, rtol=1e-4, atol=1e-3)
    _within(out, BC.mat_bound(x, w, b, act="relu", fmt=None), "matvec")  # fp32 out: no rounding stage


@pytest.mark.parametrize("B,HW,C", [(8, 65 * 65, 2048), (3, 37, 528), (2, 50, 40)])
def test_global_avgpool_i8(B, HW, C):
    """int8 NHWC global average pool (16-byte vector kernel for C % 16 == 0, byte kernel
    otherwise) against the fp32 mean of the same bytes times the scale."""
    K = _hip()
    g = torch.Generator().manual_seed(C)
    x = torch.randint(-127, 128, (B, HW, C), generator=g, dtype=torch.int32).to(torch.int8)
    out = torch.empty(B, C, device=DEV)
    ws = torch.empty(B * 16 * C, device=DEV)
    K.global_avgpool_i8(x.to(DEV), out, ws, B=B, HW=HW, C=C, scale=0.03)
    torch.cuda.synchronize()
    ref = x.double().mean(1) * 0.03
    assert torch.allclose(out.cpu().double(), ref, rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("rows,aw", [(32, 41), (1, 41), (7, 3)])
def test_pack_rows_and_copy_to_host(rows, aw):
    """The RCCL-gather send row [record | metadata] packed from a device tensor and a
    PINNED host tensor (read by the kernel over the bus), then copied back to pinned
    memory by copy_to_host: equal to the torch concatenation, bit for bit."""
    from semantic_segmentation_server_amd.ops import hip_ops
    g = torch.Generator().manual_seed(rows)
    a = torch.randn(rows, aw, generator=g)
    meta = torch.rand(rows, 3, generator=g, dtype=torch.float64).pin_memory()
    dst = torch.full((rows, aw + 6), float("nan"), device=DEV)
    hip_ops.pack_rows(dst, a.to(DEV), meta.view(torch.float32))
    host = torch.empty(rows, aw + 6).pin_memory()
    hip_ops.copy_to_host(dst, host)
    torch.cuda.synchronize()
    ref = torch.cat([a, meta.view(torch.float32)], 1)
    assert torch.equal(dst.cpu().view(torch.int32), ref.view(torch.int32))
    assert torch.equal(host.view(torch.int32), ref.view(torch.int32))
    assert torch.equal(host[:, aw:].reshape(-1).clone().view(torch.float64).view(rows, 3), meta)
    with pytest.raises(ValueError):
        hip_ops.pack_rows(dst, a.to(DEV), meta.view(torch.float32)[:, :5].contiguous())


@pytest.mark.parametrize("B,h,w,C,N", BC.ASPP_POOL)
def test_aspp_pool(B, h, w, C, N):
    """GAP + relu(W1 gap + b1) + W2 pooled in two launches vs an fp32 torch reference
    (the ASPP image-pooling branch folded into the projection's per-image bias)."""
    K = _hip()
    g = torch.Generator().manual_seed(11)
    x = (torch.randn(B, C, h, w, generator=g) + 0.3).to(torch.bfloat16)
    w1 = torch.randn(N, C, generator=g) / C ** 0.5
    b1 = torch.randn(N, generator=g)
    w2 = torch.randn(N, N, generator=g) / N ** 0.5
    ib = torch.full((B, N), float("nan"), device=DEV)
    ws = K.gap_workspace(B, C, DEV)
    K.aspp_pool(_nhwc(x).to(DEV), ws, w1.t().contiguous().to(DEV), b1.to(DEV), w2.t().contiguous().to(DEV),
                ib, B=B, HW=h * w, C=C, N=N)
    torch.cuda.synchronize()
    gref = x.float().mean((2, 3))
    ref = F.relu(gref @ w1.t() + b1) @ w2.t()
    assert _rel(ib.cpu(), ref) < 1e-4
    _within(ib, BC.aspp_pool_bound(x, w1, b1, w2), "aspp_pool")  # fp32 throughout


@pytest.mark.parametrize("variant", [0, 1, 2, 3, 4, 5, 6, 7])
@pytest.mark.parametrize("h,H,K", UR.SQUARE_SHAPES)
@pytest.mark.parametrize("field", ["noise", "smooth"])
def test_upsample_argmax(h, H, K, variant, field):
    """``smooth``: a coarse random field upsampled to h x h (large regions: the cell-bound
    variant's single-survivor path); ``noise``: i.i.d. logits (most cells keep several
    classes)."""
    from semantic_segmentation_server_amd.ops import reference_ops as R
    Kh = _hip()
    B = 2
    ldk = (K + 7) // 8 * 8
    logits = UR.square_logits(h, K, field)
    ref = R.upsample_argmax(_nchw(logits[..., :K]).float(), H, H)
    raw, out = UR.guarded(B, H, H)
    Kh.upsample_argmax(logits.to(DEV), out, B=B, h=h, w=h, K=K, ldk=ldk, H=H, W=H,
                       variant=variant)
    torch.cuda.synchronize()
    agree = (out.cpu() == ref).float().mean().item()
    assert agree > 0.9999, agree
    _labels_exact(("square", h, H, K, field), logits, raw, out, K, H, H, f"variant {variant}")


_LABEL_REF = {}


def _labels_exact(key, logits, raw, out, K, H, W, what, twin=None):
    """The float64 margin rule of tests/upsample_ref.py at EVERY pixel, and the guard rows.
    The reference of an input is computed once and shared by the variants. ``twin`` = (a, b,
    tagged): class b copies class a, so b is left out of the reference; a strict-compare
    kernel never answers b, a tagged one may answer b where the reference says a."""
    if key not in _LABEL_REF:
        a64, decided = UR.label_ref(logits.to(DEV), K, H, W, without=None if twin is None else twin[1])
        _LABEL_REF[key] = (a64.to(torch.uint8).cpu(), decided.cpu())
    a64, decided = _LABEL_REF[key]
    undecided = 1.0 - decided.double().mean().item()
    got = out.cpu()
    if twin is not None:
        a, b, tagged = twin
        if tagged:
            assert bool(((got != b) | (a64 == a) | ~decided).all()), what
            got = torch.where(got == b, torch.full_like(got, a), got)
        else:
            assert int((got == b).sum()) == 0, what
    wrong = int((got != a64)[decided].sum())
    print(f"[labels] {key} {what}: below the margin {100 * undecided:.4f} %, wrong labels {wrong}")
    assert undecided <= UR.MAX_UNDECIDED, undecided  # a condition on the test's inputs
    assert wrong == 0, (what, wrong)
    r = raw.cpu()
    assert (r[0] == UR.GUARD).all() and (r[-1] == UR.GUARD).all(), what


def _assert_path(B, h, w, H, W, K, ldk, variant, path):
    """The case's shape falls on the dispatch branch it is listed for, by ``UR.upsample_path``:
    a Python copy of the dispatch arithmetic of csrc/hip/model_ops.hip, not a report from the
    extension of the kernel that ran. It keeps a case from drifting off its branch when a
    shape is edited; what a case pins about the kernels are its labels and guard rows. The
    K 8 / ldk 8 case in particular cannot tell the dispatch fix from its absence by itself:
    the interval kernels' 32-byte over-read stays inside the allocator's block and the runtime
    K masks the channels it brings in."""
    ran = UR.upsample_path(B, h, w, H, W, K, ldk, variant)
    want = {"interval": 5 if variant == 5 else (variant or 1), "direct": 5,
            "demoted": {3: 1, 4: 2}.get(variant, 5 if variant == 5 else (variant or 1))}[path]
    assert ran == want, (ran, want)


@pytest.mark.parametrize("variant", [0, 1, 2, 3, 4, 5, 6, 7])
@pytest.mark.parametrize("B,h,w,H,W,K,ldk,path,field", [
    s[:8] + (f,) for s in UR.UPSAMPLE_SHAPES for f in (s[8] if len(s) > 8 else ("noise", "smooth"))])
def test_upsample_argmax_every_branch(B, h, w, H, W, K, ldk, path, field, variant):
    """Every dispatch branch of ``upsample_argmax`` and every variant, on small maps: labels
    equal the float64 argmax outside the margin, padding channels (+100) never win, the guard
    rows around the label plane stay untouched."""
    _assert_path(B, h, w, H, W, K, ldk, variant, path)
    if (B, w, K) == (3, 9, 19):
        assert (B * H) % (256 // w) != 0 and W % 4 != 0
    logits = UR.make_logits(B, h, w, K, ldk, field)
    raw, out = UR.guarded(B, H, W)
    _hip().upsample_argmax(logits.to(DEV), out, B=B, h=h, w=w, K=K, ldk=ldk, H=H, W=W, variant=variant)
    torch.cuda.synchronize()
    _labels_exact((B, h, w, H, W, K, ldk, field), logits, raw, out, K, H, W, f"variant {variant}")


@pytest.mark.parametrize("variant", [0, 1, 2, 3, 4, 5, 6, 7])
@pytest.mark.parametrize("B,h,w,H,W,K,ldk,path", UR.TIE_SHAPES)
def test_upsample_argmax_exact_ties(B, h, w, H, W, K, ldk, path, variant):
    """Ties need no margin. All-zero logits: label 0 everywhere. Integer logits in which
    class b copies class a < b at every source pixel: the two interpolants are bit-equal in
    any rounding order, so a first-maximum kernel (strict compare, candidate pruning) never
    answers b. The tagged variants 2 and 4 order scores closer than 2^-18 relative by their
    tag, so there only ``label in {a, b}`` is asserted. Every other pixel follows the
    margin rule."""
    _assert_path(B, h, w, H, W, K, ldk, variant, path)
    raw, out = UR.guarded(B, H, W)
    zeros = UR.make_logits(B, h, w, K, ldk, "zeros")
    _hip().upsample_argmax(zeros.to(DEV), out, B=B, h=h, w=w, K=K, ldk=ldk, H=H, W=W, variant=variant)
    torch.cuda.synchronize()
    assert int(out.max()) == 0 and (raw.cpu()[[0, -1]] == UR.GUARD).all()
    a, b = UR.TWIN
    twins = UR.make_logits(B, h, w, K, ldk, "twins")
    assert torch.equal(twins[..., a], twins[..., b])
    out.fill_(255)
    _hip().upsample_argmax(twins.to(DEV), out, B=B, h=h, w=w, K=K, ldk=ldk, H=H, W=W, variant=variant)
    torch.cuda.synchronize()
    tagged = UR.upsample_path(B, h, w, H, W, K, ldk, variant) in (2, 4)
    _labels_exact((B, h, w, H, W, K, ldk, "twins"), twins, raw, out, K, H, W, f"variant {variant}",
                  twin=(a, b, tagged))


@pytest.fixture(params=[1, 2, 0], ids=["tiles", "tiles64", "strips"])
def post_accum(request, monkeypatch):
    """Every accumulation pass of the device post-processing (LDS-staged 32 x 32 tiles,
    the default since round 4, 64 x 64 tiles, and round 3's pixel strips) must give the
    spec's records."""
    monkeypatch.setenv("SSA_POST_ACCUM", str(request.param))
    return request.param


@pytest.mark.parametrize("seed,h,w,min_area", [(0, 513, 513, 0.05 * 513 * 513), (1, 384, 513, 13158.45),
                                               (2, 97, 131, 0.0), (3, 64, 64, 10.0),
                                               (4, 200, 300, 100.0)])
def test_device_postprocess_matches_spec(seed, h, w, min_area, post_accum):
    from semantic_segmentation_server_amd.labels import pascal_colormap
    from semantic_segmentation_server_amd.postprocess.components import component_segments
    from semantic_segmentation_server_amd.postprocess.device import DevicePostprocess
    from semantic_segmentation_server_amd.postprocess.synthetic import random_label_map
    rng = np.random.default_rng(seed)
    B = 4
    H, W = max(h, 64), max(w, 64)  # model resolution; crop (h, w) inside it
    maps = np.zeros((B, H, W), np.uint8)
    for i in range(B):
        maps[i] = rng.integers(0, 21, (H, W), dtype=np.uint8)  # garbage outside the crop
        maps[i, :h, :w] = random_label_map(rng, h, w, n_blobs=int(rng.integers(1, 8)),
                                           noise=float(rng.choice([0.0, 0.01])))
    post = DevicePostprocess(torch.device(DEV), H, W, pascal_colormap(), K=64)
    rec = post.run(torch.from_numpy(maps).to(DEV), w, h, min_area)
    torch.cuda.synchronize()
    rec = rec.cpu().numpy()
    for i in range(B):
        exp = component_segments(maps[i, :h, :w], min_area, max_records=64)
        n = abs(int(rec[i, 0]))
        got = rec[i, 1:1 + 5 * n].reshape(n, 5)
        assert n == len(exp), (i, n, len(exp))
        for j in range(n):
            lab, score, area, cx, cy = exp[j][:5]
            assert int(got[j, 0]) == lab
            assert got[j, 1] == np.float32(score)
            assert got[j, 2] == np.float32(min(1.0, area / (W * H)))
            assert got[j, 3] == np.float32(min(1.0, cx / W))
            assert got[j, 4] == np.float32(min(1.0, cy / H))


@pytest.mark.parametrize("block,period,min_area", [(3, 4, 100.0), (4, 5, 100.0), (4, 5, 3000.0)])
def test_device_postprocess_many_components(block, period, min_area, post_accum):
    """Lattice masks with 10-16k components per frame (plus a few large blobs,
    the only contours above min_area): the 3x3 / period-4 lattice overflows the
    per-frame LDS merge (global union-find fallback), the others stay on the
    compact merge."""
    from semantic_segmentation_server_amd.labels import pascal_colormap
    from semantic_segmentation_server_amd.postprocess.components import component_segments
    from semantic_segmentation_server_amd.postprocess.device import DevicePostprocess
    h = w = 513
    lab = np.zeros((h, w), np.uint8)
    for y in range(0, h - block + 1, period):
        for x in range(0, w - block + 1, period):
            lab[y:y + block, x:x + block] = 15 if (x // period + y // period) % 3 else 7
    lab[40:200, 30:150] = 15
    lab[80:120, 60:100] = 0      # hole
    lab[300:480, 250:500] = 7
    lab[350:420, 300:330] = 15   # island of another class
    maps = np.stack([lab, lab[:, ::-1].copy()])
    post = DevicePostprocess(torch.device(DEV), h, w, pascal_colormap(), K=64)
    rec = post.run(torch.from_numpy(maps).to(DEV), w, h, min_area).cpu().numpy()
    for i in range(2):
        exp = component_segments(maps[i], min_area, max_records=64)
        n = abs(int(rec[i, 0]))
        assert n == len(exp), (n, len(exp))
        got = rec[i, 1:1 + 5 * n].reshape(n, 5)
        for j in range(n):
            lab_, score, area, cx, cy = exp[j][:5]
            assert int(got[j, 0]) == lab_ and got[j, 1] == np.float32(score)
            assert got[j, 2] == np.float32(min(1.0, area / (w * h)))
            assert got[j, 3] == np.float32(min(1.0, cx / w))
            assert got[j, 4] == np.float32(min(1.0, cy / h))


def test_device_postprocess_pool_exhausted():
    """32 lattice frames of ~16k components each overflow the batch's root pool
    (max(B * 8192, H * W + 1) + H * W / 2 + 1 entries): the frames that did not fit come
    back with a NaN count, every frame that did is exact, and the next call starts from an
    empty pool again."""
    from semantic_segmentation_server_amd.labels import pascal_colormap
    from semantic_segmentation_server_amd.postprocess.components import component_segments
    from semantic_segmentation_server_amd.postprocess.device import DevicePostprocess
    h = w = 513
    lab = np.zeros((h, w), np.uint8)
    for y in range(0, h - 2, 4):
        for x in range(0, w - 2, 4):
            lab[y:y + 3, x:x + 3] = 15
    lab[40:200, 30:150] = 15
    B = 32
    maps = np.broadcast_to(lab, (B, h, w)).copy()
    exp = component_segments(lab, 100.0, max_records=64)
    post = DevicePostprocess(torch.device(DEV), h, w, pascal_colormap(), K=64)
    lost = []
    for _ in range(2):
        rec = post.run(torch.from_numpy(maps).to(DEV), w, h, 100.0).cpu().numpy()
        nan = np.isnan(rec[:, 0])
        lost.append(int(nan.sum()))
        assert 0 < lost[-1] < B, lost
        for i in np.nonzero(~nan)[0]:
            n = abs(int(rec[i, 0]))
            assert n == len(exp), (i, n, len(exp))
            got = rec[i, 1:1 + 5 * n].reshape(n, 5)
            for j in range(n):
                assert int(got[j, 0]) == exp[j][0] and got[j, 1] == np.float32(exp[j][1])
                assert got[j, 3] == np.float32(min(1.0, exp[j][3] / w))
    assert lost[0] == lost[1]


def test_device_postprocess_two_lattice_frames_fit():
    """two union-find-fallback (lattice) frames in one batch beside ordinary
    ones all fit the root pool (its N + 1 floor beyond the shared part) and are exact."""
    from semantic_segmentation_server_amd.labels import pascal_colormap
    from semantic_segmentation_server_amd.postprocess.components import component_segments
    from semantic_segmentation_server_amd.postprocess.device import DevicePostprocess
    h = w = 513
    lat = np.zeros((h, w), np.uint8)
    for y in range(0, h - 2, 4):
        for x in range(0, w - 2, 4):
            lat[y:y + 3, x:x + 3] = 15
    lat[40:200, 30:150] = 15
    plain = np.zeros((h, w), np.uint8)
    plain[100:300, 50:250] = 7
    plain[350:420, 300:480] = 15
    B = 8
    maps = np.stack([lat if i in (2, 5) else plain for i in range(B)])
    post = DevicePostprocess(torch.device(DEV), h, w, pascal_colormap(), K=64)
    rec = post.run(torch.from_numpy(maps).to(DEV), w, h, 100.0).cpu().numpy()
    assert not np.isnan(rec[:, 0]).any(), rec[:, 0]
    for i in range(B):
        exp = component_segments(maps[i], 100.0, max_records=64)
        n = abs(int(rec[i, 0]))
        assert n == len(exp), (i, n, len(exp))
        got = rec[i, 1:1 + 5 * n].reshape(n, 5)
        for j in range(n):
            assert int(got[j, 0]) == exp[j][0] and got[j, 1] == np.float32(exp[j][1])


@pytest.mark.parametrize("K", [8, 64])
def test_device_postprocess_overflow_deterministic(K, post_accum):
    """More contours pass min_area than there are record slots: the device keeps the
    first K by discovery key (same rule as the spec's ``max_records``), flags the frame
    with a negative count, and gives identical records on every run."""
    from semantic_segmentation_server_amd.labels import pascal_colormap
    from semantic_segmentation_server_amd.postprocess.components import component_segments
    from semantic_segmentation_server_amd.postprocess.device import DevicePostprocess
    h = w = 257
    lab = np.zeros((h, w), np.uint8)
    rng = np.random.default_rng(5)
    for y in range(2, h - 12, 14):       # ~300 blobs of 6-10 px, classes 7 / 15
        for x in range(2, w - 12, 14):
            s_ = int(rng.integers(6, 11))
            lab[y:y + s_, x:x + s_] = 15 if rng.random() < 0.5 else 7
    lab[100:140, 100:160] = 0            # a hole inside nothing (background) - no-op
    maps = np.stack([lab, lab[::-1].copy(), np.zeros_like(lab)])
    post = DevicePostprocess(torch.device(DEV), h, w, pascal_colormap(), K=K)
    outs = []
    for _ in range(3):
        outs.append(post.run(torch.from_numpy(maps).to(DEV), w, h, 10.0).cpu().numpy().copy())
    for o in outs[1:]:
        assert np.array_equal(o, outs[0])
    rec = outs[0]
    for i in range(2):
        full = component_segments(maps[i], 10.0)
        assert len(full) > K
        exp = component_segments(maps[i], 10.0, max_records=K)
        assert int(rec[i, 0]) == -len(exp)   # overflow flag: negative count
        got = rec[i, 1:1 + 5 * K].reshape(K, 5)
        for j in range(K):
            lab_, score, area, cx, cy = exp[j][:5]
            assert int(got[j, 0]) == lab_ and got[j, 1] == np.float32(score)
            assert got[j, 3] == np.float32(min(1.0, cx / w)) and got[j, 4] == np.float32(min(1.0, cy / h))
    assert rec[2, 0] == 0


def test_device_postprocess_deep_nesting(post_accum):
    """Concentric 3-px rings nest ~80 contours deep (> the 32-entry ancestor chains of
    k_finalize): the record order must still be findContours pre-order."""
    from semantic_segmentation_server_amd.labels import pascal_colormap
    from semantic_segmentation_server_amd.postprocess.components import component_segments
    from semantic_segmentation_server_amd.postprocess.device import DevicePostprocess
    h = w = 257
    yy, xx = np.mgrid[0:h, 0:w]
    ring = np.maximum(np.abs(yy - 128), np.abs(xx - 128)) // 3
    lab = np.where(ring % 2 == 0, 15, 0).astype(np.uint8)
    lab[:, :] = np.where(ring >= 42, 0, lab)
    maps = lab[None].copy()
    post = DevicePostprocess(torch.device(DEV), h, w, pascal_colormap(), K=128)
    rec = post.run(torch.from_numpy(maps).to(DEV), w, h, 0.0).cpu().numpy()
    exp = component_segments(lab, 0.0, max_records=128)
    assert len(exp) > 40, len(exp)
    n = abs(int(rec[0, 0]))
    assert n == len(exp)
    got = rec[0, 1:1 + 5 * n].reshape(n, 5)
    for j in range(n):
        lab_, score, area, cx, cy = exp[j][:5]
        assert int(got[j, 0]) == lab_ and got[j, 1] == np.float32(score), j
        assert got[j, 2] == np.float32(min(1.0, area / (w * h))), j


def _small_cfg(**kw):
    from semantic_segmentation_server_amd import config as C
    base = dict(input_size=129, batch=2, backend="hip", graph=False)
    base.update(kw)
    return C.Config(**base)


@pytest.mark.parametrize("B", [32, 16, 8, 1])
def test_hip_model_headline_shape_matches_torch(B):
    """The headline shape (513^2, 640x480 camera) with the committed MI355X picks of that
    batch size -- B = 32 is the plan bench.py runs, B = 1 the batch-1 /
    latency plan: grids large enough that several workgroups of a kernel share a CU (the
    small-shape test below runs most kernels at one workgroup per CU). Bound relative to
    stock PyTorch bf16 on the same GPU, as below, plus the argmax agreement."""
    from semantic_segmentation_server_amd.models.deeplab import build_model
    from semantic_segmentation_server_amd.models.hip_model import TUNE_FILE_DEFAULT, HipDeepLab
    from semantic_segmentation_server_amd.ops import reference_ops as R
    import json
    S = 513
    assert f"mnv2:B={B}:cam=640x480:in=513" in json.load(open(TUNE_FILE_DEFAULT))
    model = build_model("mnv2", 21, calibrate_hw=129)
    cfg = _small_cfg(input_size=S)
    hm = HipDeepLab(model, torch.device(DEV), cfg)
    lx, ly, *_ = R.letterbox_luts(640, 480, S, S)
    rng = np.random.default_rng(9)
    frames = torch.from_numpy(rng.integers(0, 256, (B, 480, 640, 3), dtype=np.uint8))
    x = R.preprocess(frames, lx, ly).to(DEV)
    import copy
    with torch.no_grad():
        ref_logits = copy.deepcopy(model).to(DEV)(x).float().cpu()
        bf_logits = copy.deepcopy(model).to(DEV, torch.bfloat16)(x.to(torch.bfloat16)).float().cpu()
    dl = hm.logits(frames.to(DEV), torch.tensor(lx, device=DEV), torch.tensor(ly, device=DEV))
    torch.cuda.synchronize()
    saved = json.load(open(TUNE_FILE_DEFAULT))[f"mnv2:B={B}:cam=640x480:in=513"]
    assert all(saved.get(n) == v for n, v in hm.choices.items() if n in saved), \
        "the plan under test is not the committed one"
    got = _nchw(dl.float()).cpu()
    e_hip, e_bf = _rel(got, ref_logits), _rel(bf_logits, ref_logits)
    print(f"headline shape B={B}: rel err hip={e_hip:.4f} torch-bf16={e_bf:.4f}")
    # no less accurate than stock PyTorch bf16 on the same GPU (the old
    # 1.5x + 0.01 bound left 3.6x headroom), with an absolute ceiling
    assert e_hip < 1.0 * e_bf + 0.005 and e_hip < 0.1, (e_hip, e_bf)
    ref_lab = R.upsample_argmax(ref_logits, S, S)
    hip_lab = R.upsample_argmax(got, S, S)
    bf_lab = R.upsample_argmax(bf_logits, S, S)
    a_hip = (hip_lab == ref_lab).float().mean().item()
    a_bf = (bf_lab == ref_lab).float().mean().item()
    d_hip, frac = R.decisive_agreement(got, ref_logits)
    print(f"  argmax agreement with fp32: hip={a_hip:.4f} torch-bf16={a_bf:.4f}; "
          f"decisive pixels ({frac:.3f} of all) hip={d_hip:.4f}")
    # plain argmax agreement is near-tie noise with random-init weights (torch-bf16 itself
    # measured 0.77 and 0.90 on this frame in two processes); decisions with a margin of
    # several error-sigmas must hold
    assert d_hip >= 0.995 and frac > 0.05, (d_hip, frac)
    # deterministic: a second run of the same plan gives the same logits bit for bit
    dl2 = hm.logits(frames.to(DEV), torch.tensor(lx, device=DEV), torch.tensor(ly, device=DEV))
    torch.cuda.synchronize()
    assert torch.equal(_nchw(dl2.float()).cpu(), got)


@pytest.mark.parametrize("arch,aspp", [("mnv2", "full"), ("mnv2", "mobile"), ("resnet50", "full")])
def test_hip_model_matches_torch(arch, aspp):
    """Whole network vs the fp32 torch model. bf16 activations drift over ~60
    layers, so the bound is relative to stock PyTorch running the same model in
    bf16 on the same GPU: the HIP path must be no less accurate than that."""
    from semantic_segmentation_server_amd.models.deeplab import build_model
    from semantic_segmentation_server_amd.models.hip_model import HipDeepLab
    from semantic_segmentation_server_amd.ops import reference_ops as R
    S = 129
    nc = 21 if arch == "mnv2" else 19
    model = build_model(arch, nc, aspp=aspp, calibrate_hw=65)
    cfg = _small_cfg(arch=arch, aspp=aspp)
    hm = HipDeepLab(model, torch.device(DEV), cfg)
    lx, ly, *_ = R.letterbox_luts(160, 120, S, S)
    rng = np.random.default_rng(8)
    frames = torch.from_numpy(rng.integers(0, 256, (2, 120, 160, 3), dtype=np.uint8))
    x = R.preprocess(frames, lx, ly)
    with torch.no_grad():
        ref_logits = model(x)  # fp32 CPU
        import copy
        mb = copy.deepcopy(model).to(DEV, torch.bfloat16)
        bf_logits = mb(x.to(DEV, torch.bfloat16)).float().cpu()
    dl = hm.logits(frames.to(DEV), torch.tensor(lx, device=DEV), torch.tensor(ly, device=DEV))
    torch.cuda.synchronize()
    got = _nchw(dl.float()).cpu()
    assert got.shape == ref_logits.shape
    e_hip, e_bf = _rel(got, ref_logits), _rel(bf_logits, ref_logits)
    print(f"{arch}/{aspp}: rel err hip={e_hip:.4f} torch-bf16={e_bf:.4f}")
    assert e_hip < 1.0 * e_bf + 0.005, (e_hip, e_bf)
    labels = hm.segment(frames.to(DEV), torch.tensor(lx, device=DEV), torch.tensor(ly, device=DEV))
    ref_lab = R.upsample_argmax(ref_logits, S, S)
    bf_lab = R.upsample_argmax(bf_logits, S, S)
    a_hip = (labels.cpu() == ref_lab).float().mean().item()
    a_bf = (bf_lab == ref_lab).float().mean().item()
    print(f"  argmax agreement with fp32: hip={a_hip:.4f} torch-bf16={a_bf:.4f}")
    assert a_hip > a_bf - 0.02


def test_engine_graph_replay_matches_eager():
    from semantic_segmentation_server_amd.runtime.engine import Engine
    from semantic_segmentation_server_amd.runtime.sources import SyntheticSource
    cfg = _small_cfg(graph=True)
    eng = Engine(cfg, torch.device(DEV))
    src = SyntheticSource(200, 150, pool=4)
    f1, _, _ = src.read_batch(2)
    f2, _, _ = src.read_batch(2)
    eng.set_camera(200, 150)
    d1 = torch.from_numpy(f1).to(DEV)
    d2 = torch.from_numpy(f2).to(DEV)
    eager1 = eng._infer_eager(d1).clone()
    eager2 = eng._infer_eager(d2).clone()
    g1, p1 = eng.run_device(d1)
    g1 = g1.clone()
    g2, p2 = eng.run_device(d2)  # replay after input mutation
    torch.cuda.synchronize()
    assert torch.equal(g1, eager1)
    assert torch.equal(g2, eager2)
    assert p2 is not None and p2.shape == (2, 1 + 5 * cfg.max_segments)


@pytest.mark.parametrize("split", [False, True])
def test_engine_bound_input_graphs(split):
    """bind_inputs: a graph per persistent input buffer reads it in place; results
    equal the eager step, alternating between the buffers after they are refilled.
    split: model and post-processing graphs on two streams (records on result_stream)."""
    from semantic_segmentation_server_amd.runtime.engine import Engine
    from semantic_segmentation_server_amd.runtime.sources import SyntheticSource
    cfg = _small_cfg(graph=True)
    eng = Engine(cfg, torch.device(DEV))
    eng.set_camera(200, 150)
    src = SyntheticSource(200, 150, pool=4, seed=3)
    bufs = [torch.empty((2, 150, 200, 3), dtype=torch.uint8, device=DEV) for _ in range(2)]
    eng.bind_inputs(bufs, split_post=split)
    for it in range(3):
        for b in bufs:
            f, _, _ = src.read_batch(2)
            b.copy_(torch.from_numpy(f))
            torch.cuda.synchronize()
            want = eng._infer_eager(b).clone()
            want_post = eng._device_post(want).clone()
            torch.cuda.synchronize()
            got, post = eng.run_device(b)
            torch.cuda.synchronize()
            assert torch.equal(got, want), it
            assert _records_equal(post, want_post), it
    # pipelined: both slots in flight before anything is read back
    outs = []
    for b in bufs:
        got, post = eng.run_device(b)
        rs = getattr(eng, "result_stream", None) or torch.cuda.current_stream()
        with torch.cuda.stream(rs):
            outs.append((got.clone(), post.clone()))
    torch.cuda.synchronize()
    for (got, post), b in zip(outs, bufs):
        want = eng._infer_eager(b).clone()
        assert torch.equal(got, want) and _records_equal(post, eng._device_post(want))
    assert len(eng._bound_graphs) == 2

    def check(frames):
        f, _, _ = src.read_batch(2)
        frames.copy_(torch.from_numpy(f))
        torch.cuda.synchronize()
        want = eng._infer_eager(frames).clone()
        want_post = eng._device_post(want).clone()
        torch.cuda.synchronize()
        got, post = eng.run_device(frames)
        torch.cuda.synchronize()
        assert torch.equal(got, want) and _records_equal(post, want_post)

    # an unbound tensor of the same shape takes the static input's step beside the bound ones
    check(torch.empty_like(bufs[0]))
    assert len(eng._bound_graphs) == 2
    # a camera change drops the bound steps: new buffers run the new letterbox, the old are gone
    eng.set_camera(160, 120)
    src = SyntheticSource(160, 120, pool=4, seed=3)
    bufs = [torch.empty((2, 120, 160, 3), dtype=torch.uint8, device=DEV) for _ in range(2)]
    eng.bind_inputs(bufs, split_post=split)
    for b in bufs:
        check(b)
    assert len(eng._bound_graphs) == 2


@pytest.mark.parametrize("ingest", ["local", "scatter"])
def test_rccl_world1_pipeline_records_match_eager(ingest):
    """The RCCL data path (RCCL process group + gloo control group, RCCL
    record gather, lag 2 slot-parallel; with ``scatter`` also the RCCL frame scatter on
    the slot streams) rehearsed at world size 1 on this GPU (SSA_FORCE_PG=1): records
    equal the eager engine's (scripts/rccl_world1_check.py, in a child process so its
    process group does not leak into other tests)."""
    import os
    import socket
    import subprocess
    import sys
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, SSA_FORCE_PG="1", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
               WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, os.path.join(root, "scripts", "rccl_world1_check.py"), ingest],
                       env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert f"OK ingest={ingest} gather=rccl pg=nccl lag=2" in r.stdout, r.stdout


@pytest.mark.parametrize("lag", [0, 1, 2])
def test_dp_pipeline_records_match_eager(lag):
    """The DP pipeline (bound per-slot graphs; lag 1: split model / post graphs on two
    streams, records collected one step late) returns, over many steps of two
    alternating batches with planted person/car regions, exactly the records of an
    eager, synchronous engine on the same frames."""
    from semantic_segmentation_server_amd.parallel import dist as D
    from semantic_segmentation_server_amd.parallel.dp import DataParallelPipeline
    from semantic_segmentation_server_amd.runtime.engine import Engine
    from semantic_segmentation_server_amd.runtime.sources import SyntheticSource
    kw = dict(batch=2, input_size=257, min_area_ratio=0.002)
    eng = Engine(_small_cfg(graph=True, **kw), torch.device(DEV))
    src = SyntheticSource(160, 120, seed=7, pool=4)
    batches = [torch.from_numpy(np.ascontiguousarray(src.read_batch(2)[0])) for _ in range(2)]
    # expected: the same engine's eager (ungraphed, single-stream) step -- same weights and
    # the same autotuned kernel picks, so the records must match exactly
    eng.set_camera(160, 120)
    want = []
    for k in range(6):
        f = batches[k % 2].to(DEV)
        _, post = eng._step_device(f)
        r = eng._hip_post.fetch(post, [k * 2, k * 2 + 1], [0.0, 0.0], [0, 0], eng.W, eng.H)
        want.append(sorted(zip(r["frame"].tolist(), r["label"].tolist(), r["area"].round(6).tolist())))
    torch.cuda.synchronize()
    ctx = D.init()
    pipe = DataParallelPipeline(ctx, eng, 160, 120, 2, "local", None, lag=lag)
    got_all = []
    pipe.prefetch(batches[0].pin_memory())
    for k in range(6):
        recs = pipe.step(next_frames=batches[(k + 1) % 2].pin_memory() if k < 5 else None)
        got_all.extend(zip(recs["frame"].tolist(), recs["label"].tolist(), recs["area"].round(6).tolist()))
    last = pipe.flush()
    got_all.extend(zip(last["frame"].tolist(), last["label"].tolist(), last["area"].round(6).tolist()))
    torch.cuda.synchronize()
    assert sum(len(w) for w in want) > 0  # the frames do produce contours
    assert sorted(got_all) == sorted(x for w in want for x in w)


def _race_setup(B=2, S=257, cam=(160, 120)):
    from semantic_segmentation_server_amd.runtime.engine import Engine
    from semantic_segmentation_server_amd.runtime.sources import SyntheticSource
    eng = Engine(_small_cfg(graph=True, batch=B, input_size=S, min_area_ratio=0.002), torch.device(DEV))
    src = SyntheticSource(cam[0], cam[1], seed=7, pool=4)
    eng.set_camera(*cam)
    frames = [torch.from_numpy(np.ascontiguousarray(src.read_batch(B)[0])).to(DEV) for _ in range(3)]
    return eng, eng._hip_model, frames


def test_concurrent_plan_copies_bit_identical():
    """Three plan copies of the HIP model on three streams at once (the slot-parallel
    situation: kernels of different copies share CUs and SIMDs) give exactly the label
    maps of sequential runs, frame for frame. Round 2 saw 3-10 mismatches per 450-600
    runs here; the cause was packed-f32 VALU results corrupted under co-residence
    (profiles/r3_packed_f32_race.txt), which the build now disables."""
    eng, hm, fr = _race_setup()
    for part in range(3):
        hm.segment(fr[0], eng.lut_x, eng.lut_y, part=part)
    ref = [hm.segment(f, eng.lut_x, eng.lut_y, part=0).clone() for f in fr]
    torch.cuda.synchronize()
    ss = [torch.cuda.Stream() for _ in range(3)]
    labs = [torch.empty_like(ref[0]) for _ in range(3)]
    bad = torch.zeros((), dtype=torch.int64, device=DEV)
    for rep in range(60):
        for part in range(3):
            with torch.cuda.stream(ss[part]):
                hm.segment(fr[(rep + part) % 3], eng.lut_x, eng.lut_y, out=labs[part], part=part)
        torch.cuda.synchronize()
        for part in range(3):
            bad += (labs[part] != ref[(rep + part) % 3]).any()
    torch.cuda.synchronize()
    assert int(bad) == 0, f"{int(bad)} of 180 concurrent runs differ from the sequential label maps"


@pytest.mark.parametrize("shape", ["257", "headline"])
def test_plan_is_a_function_of_the_frame(shape, tmp_path, monkeypatch):
    """The default plan's label maps depend on the frame alone: the same frame after two
    different predecessor frames (and after its plan buffers were NaN-filled) gives
    bit-identical labels (no history-dependent reads). ``headline``:
    513^2 / 640x480 at B = 2 with the committed B = 32 picks (the kernels the headline runs:
    stream spans, hidden-split bands, grouped ASPP), choices whose B = 32 variant has no
    B = 2 counterpart timed afresh."""
    if shape == "headline":
        import json
        from semantic_segmentation_server_amd.models.hip_model import TUNE_FILE_DEFAULT
        picks = json.load(open(TUNE_FILE_DEFAULT))["mnv2:B=32:cam=640x480:in=513"]
        tf = tmp_path / "tune.json"
        tf.write_text(json.dumps({"mnv2:B=2:cam=640x480:in=513": picks}))
        monkeypatch.setenv("SSA_TUNE_FILE", str(tf))
        eng, hm, fr = _race_setup(2, 513, (640, 480))
        cam = (480, 640)
    else:
        eng, hm, fr = _race_setup()
        cam = (120, 160)
    a = [hm.segment(fr[0], eng.lut_x, eng.lut_y).clone()]
    hm.segment(fr[1], eng.lut_x, eng.lut_y)
    a.append(hm.segment(fr[0], eng.lut_x, eng.lut_y).clone())
    hm.segment(fr[2], eng.lut_x, eng.lut_y)
    a.append(hm.segment(fr[0], eng.lut_x, eng.lut_y).clone())
    if shape == "headline":  # the picks that ran are the headline's where the names exist
        want = json.load(open(TUNE_FILE_DEFAULT))["mnv2:B=32:cam=640x480:in=513"]
        same = [n for n, v in hm.choices.items() if want.get(n) == v]
        assert any(v.startswith("stream") for v in hm.choices.values()), hm.choices
        assert len(same) >= len(want) // 2, (same, hm.choices)
    _, bufs = hm._plan(2, *cam)
    for n, t in bufs.items():  # activation buffers only (int tables are plan constants)
        if not isinstance(t, torch.Tensor) or not t.is_cuda or n.startswith(("pool_w", "aspp_proj_wt", "const_")):
            continue
        if t.dtype == torch.uint8:
            t.fill_(0xC0)
        elif t.dtype == torch.float32:
            t.view(torch.int32).fill_(0x7FC07FC0)
        elif t.dtype in (torch.bfloat16, torch.float16):
            t.view(torch.int16).fill_(0x7FC0)
    a.append(hm.segment(fr[0], eng.lut_x, eng.lut_y).clone())
    torch.cuda.synchronize()
    assert all(torch.equal(a[0], x) for x in a[1:])


def test_hip_backend_rejects_fp32():
    from semantic_segmentation_server_amd.runtime.engine import Engine
    with pytest.raises(ValueError, match="fp32"):
        Engine(_small_cfg(dtype="fp32"), torch.device(DEV))


@pytest.mark.parametrize("parts", [2, 4, "slot"])
def test_dp_pipeline_model_parts_match_eager(monkeypatch, parts):
    """SSA_MODEL_PARTS=P: each step's model runs as P concurrent sub-batch graphs on P
    streams and each part's post-processing starts as soon as its labels exist; the
    records must equal those of eager, synchronous per-part steps (the part plans' own
    kernel picks)."""
    from semantic_segmentation_server_amd.parallel import dist as D
    from semantic_segmentation_server_amd.parallel.dp import DataParallelPipeline
    from semantic_segmentation_server_amd.runtime.engine import Engine
    from semantic_segmentation_server_amd.runtime.sources import SyntheticSource
    slot = parts == "slot"  # SSA_SLOT_PARALLEL: one plan copy + model stream per staging slot
    monkeypatch.setenv("SSA_SLOT_PARALLEL", "1" if slot else "0")
    if slot:
        parts = 1
    monkeypatch.setenv("SSA_MODEL_PARTS", str(parts))
    n = 2 * parts  # two frames per part
    kw = dict(batch=n, input_size=257, min_area_ratio=0.002)
    eng = Engine(_small_cfg(graph=True, **kw), torch.device(DEV))
    src = SyntheticSource(160, 120, seed=7, pool=4)
    batches = [torch.from_numpy(np.ascontiguousarray(src.read_batch(n)[0])) for _ in range(2)]
    eng.set_camera(160, 120)
    want = []
    for k in range(6):
        f = batches[k % 2].to(DEV)
        for h in range(parts):
            lab = eng._hip_model.segment(f[2 * h:2 * h + 2], eng.lut_x, eng.lut_y, part=0)
            post = eng._device_post(lab)
            ids = [k * n + 2 * h, k * n + 2 * h + 1]
            r = eng._hip_post.fetch(post, ids, [0.0, 0.0], [0, 0], eng.W, eng.H)
            want.extend(zip(r["frame"].tolist(), r["label"].tolist(), r["area"].round(6).tolist()))
    torch.cuda.synchronize()
    ctx = D.init()
    pipe = DataParallelPipeline(ctx, eng, 160, 120, n, "local", None, lag=1)
    assert eng.model_parts == parts
    got = []
    pipe.prefetch(batches[0].pin_memory())
    for k in range(6):
        recs = pipe.step(next_frames=batches[(k + 1) % 2].pin_memory() if k < 5 else None)
        got.extend(zip(recs["frame"].tolist(), recs["label"].tolist(), recs["area"].round(6).tolist()))
    last = pipe.flush()
    got.extend(zip(last["frame"].tolist(), last["label"].tolist(), last["area"].round(6).tolist()))
    torch.cuda.synchronize()
    if slot:
        assert len(eng.slot_streams) == pipe.nslots  # each staging slot ran on its own stream
    else:
        assert len(eng.model_streams) == parts - 1  # the parts path ran
    assert len(want) > 0
    assert sorted(got) == sorted(want)


def test_engine_step_records_flow():
    from semantic_segmentation_server_amd.runtime.engine import Engine
    from semantic_segmentation_server_amd.runtime.sources import SyntheticSource
    eng = Engine(_small_cfg(graph=True), torch.device(DEV))
    src = SyntheticSource(320, 240, pool=2)
    frames, ids, ts = src.read_batch(2)
    recs = eng.step(frames, ids, ts, 0)
    assert recs.dtype.names[0] == "label"


@pytest.mark.parametrize("cin,cout,t,stride,H", BC.FUSED_IR)
def test_fused_inverted_residual(cin, cout, t, stride, H):
    from semantic_segmentation_server_amd.models.layers import init_random
    from semantic_segmentation_server_amd.models.mobilenetv2 import InvertedResidual, IRSpec
    K = _hip()
    spec = IRSpec(cin, cout, t, stride, 1)
    blk = InvertedResidual(spec)
    init_random(blk, seed=cin + cout)
    for m in blk.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_mean.uniform_(-0.2, 0.2)
            m.running_var.uniform_(0.5, 2.0)
    blk.eval()
    g = torch.Generator().manual_seed(9)
    B, W = 2, H + 6
    x = torch.randn(B, cin, H, W, generator=g).to(torch.bfloat16)
    with torch.no_grad():
        ref = blk(x.float())
    OH, OW = ref.shape[-2:]
    ew = eb = None
    if blk.expand is not None:
        ew, eb = blk.expand.fold()
        ew = ew[:, :, 0, 0]
    dwf, dbf = blk.dw.fold()
    pwf, pbf = blk.project.fold()
    packed = K.pack_fused_ir(ew, eb, dwf[:, 0], dbf, pwf[:, :, 0, 0], pbf, Cin=cin, hid=spec.hidden,
                             Cout=cout, stride=stride, residual=spec.residual, device=DEV)
    raw, out = _guarded_out((B, OH, OW, cout), 7.0)
    K.fused_ir(_nhwc(x).to(DEV), packed, out, B=B, IH=H, IW=W, OH=OH, OW=OW)
    torch.cuda.synchronize()
    assert _rel(_nchw(out).cpu(), ref) < 2e-2
    _within(_nchw(out), BC.fused_ir_bound(x, packed, tile=False), "fused_ir row kernel")
    assert _guards_kept(raw, 7.0)


def _stem_block0_case(cam, H, seed, with_refs):
    """The inputs of a stem + block 0 test on the device (tests/bound_cases.py) and, where
    asked for, the fp32 torch layers' output and the float64 reference pair, computed once per
    (camera, map size, frame seed) and shared by every tile / band parametrisation."""
    from semantic_segmentation_server_amd.ops import reference_ops as R

    def make():
        stem, blk, frames, lx, ly, P = BC.stem_block0_case(cam, H, seed, DEV)
        ref = bound = None
        if with_refs:
            x = R.preprocess(frames, torch.from_numpy(np.array(lx)), torch.from_numpy(np.array(ly)))
            with torch.no_grad():
                ref = blk(stem(x))
            bound = BC.stem_block0_bound(BC.stem_pixels(frames, lx, ly, True), P)
        return (frames.to(DEV), torch.tensor(np.array(lx), dtype=torch.int32, device=DEV),
                torch.tensor(np.array(ly), dtype=torch.int32, device=DEV), P, ref, bound)
    return _bound(("stem_block0", cam, H, seed), make)


@pytest.mark.parametrize("cam,H,tile", BC.STEM_BLOCK0)
def test_stem_block0_fused(cam, H, tile):
    K = _hip()
    fd, lxd, lyd, P, ref, bound = _stem_block0_case(cam, H, 3, True)
    SH = (H - 1) // 2 + 1
    out = torch.full((2, SH, SH, 16), float("nan"), dtype=torch.bfloat16, device=DEV)
    K.stem_block0(fd, lxd, lyd, P, out, H=H, W=H, tile=tile)
    torch.cuda.synchronize()
    assert torch.isfinite(out).all()
    assert _rel(_nchw(out).cpu(), ref) < 2e-2
    _within(_nchw(out), bound, f"stem_block0 tile {tile}")


@pytest.mark.parametrize("cam,H", BC.STEM_BAND)
@pytest.mark.parametrize("R,nbx", [(16, 3), (5, 4), (33, 5), (7, 1), (300, 2)])
def test_stem_band(cam, H, R, nbx):
    """Row-streaming stem + block 0: bit-identical to the tile kernel (same arithmetic:
    one gather per input pixel, one stem evaluation per stem pixel, depthwise bias-first in
    tap order), incl. the letterbox LUT path (letterbox rows below the frame, a portrait
    camera letterboxed on the right) and bands cut at the image borders; and vs the fp32
    torch layers."""
    K = _hip()
    SH = (H - 1) // 2 + 1
    if -(-(-(-SH // nbx) + 2) // 16) > 8:
        pytest.skip("band wider than 8 column groups")
    fd, lxd, lyd, P, ref, bound = _stem_block0_case(cam, H, 4, H <= BC.STEM_BAND_MAX_H)
    want = torch.full((2, SH, SH, 16), float("nan"), dtype=torch.bfloat16, device=DEV)
    K.stem_block0(fd, lxd, lyd, P, want, H=H, W=H, tile=(8, 16))
    for oneb in (True, False):  # one barrier per stem row (double-buffered row) / two
        out = torch.full((2, SH, SH, 16), float("nan"), dtype=torch.bfloat16, device=DEV)
        K.stem_band(fd, lxd, lyd, P, out, H=H, W=H, R=R, nbx=nbx, one_barrier=oneb)
        torch.cuda.synchronize()
        assert torch.isfinite(out).all(), oneb
        assert torch.equal(out, want), (oneb, (out.float() - want.float()).abs().max().item())
    if H <= BC.STEM_BAND_MAX_H:
        assert _rel(_nchw(out).cpu(), ref) < 2e-2
        # out equals the tile kernel's output bit for bit (above); the 513 maps are bounded there
        _within(_nchw(out), bound, f"stem_band R {R} nbx {nbx}")


@pytest.mark.parametrize("cin,cout,stride,dil,H,tile", BC.FUSED_IR_TILE)
def test_fused_ir_tile(cin, cout, stride, dil, H, tile):
    from semantic_segmentation_server_amd.models.layers import init_random
    from semantic_segmentation_server_amd.models.mobilenetv2 import InvertedResidual, IRSpec
    K = _hip()
    spec = IRSpec(cin, cout, 1 if cout == 16 else 6, stride, dil)
    blk = InvertedResidual(spec)
    init_random(blk, seed=cin + 3 * cout + dil)
    for m in blk.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_mean.uniform_(-0.2, 0.2)
            m.running_var.uniform_(0.5, 2.0)
    blk.eval()
    g = torch.Generator().manual_seed(19)
    B, W = 2, H + 4
    x = torch.randn(B, cin, H, W, generator=g).to(torch.bfloat16)
    with torch.no_grad():
        ref = blk(x.float())
    OH, OW = ref.shape[-2:]
    ew = eb = None
    if blk.expand is not None:
        ew, eb = blk.expand.fold()
        ew = ew[:, :, 0, 0]
    dwf, dbf = blk.dw.fold()
    pwf, pbf = blk.project.fold()
    packed = K.pack_fused_ir(ew, eb, dwf[:, 0], dbf, pwf[:, :, 0, 0], pbf, Cin=cin,
                             hid=spec.hidden, Cout=cout, stride=stride, residual=spec.residual,
                             device=DEV, dil=dil)
    raw, out = _guarded_out((B, OH, OW, cout), float("nan"))
    K.fused_ir(_nhwc(x).to(DEV), packed, out, B=B, IH=H, IW=W, OH=OH, OW=OW, tile=tile)
    torch.cuda.synchronize()
    assert torch.isfinite(out).all()
    assert _rel(_nchw(out).cpu(), ref) < 2e-2
    _within(_nchw(out), BC.fused_ir_bound(x, packed, tile=True), f"fused_ir tile kernel {tile}")
    assert _guards_kept(raw, float("nan"))


@pytest.mark.parametrize("hid,cout,stride,dil,res", BC.DW_PROJECT)
def test_dw_project(hid, cout, stride, dil, res):
    K = _hip()
    g = torch.Generator().manual_seed(10)
    B, H = 2, 21
    x = F.relu6(torch.randn(B, hid, H, H, generator=g) * 2).to(torch.bfloat16)
    wd = torch.randn(hid, 1, 3, 3, generator=g) / 3
    bd = torch.randn(hid, generator=g) * 0.1
    wp = torch.randn(cout, hid, generator=g) / hid ** 0.5
    bp = torch.randn(cout, generator=g) * 0.1
    d = F.relu6(F.conv2d(x.float(), wd, bd, stride, dil, dil, groups=hid)).to(torch.bfloat16).float()
    ref = F.conv2d(d, wp.to(torch.bfloat16).float()[:, :, None, None], bp)
    OH, OW = ref.shape[-2:]
    r = torch.randn(B, cout, OH, OW, generator=g).to(torch.bfloat16) if res else None
    if res:
        ref = ref + r.float()
    wpp, bpp = K.pack_project_padded(wp, bp, cout, hid, DEV)
    raw, out = _guarded_out((B, OH, OW, cout), 7.0)
    K.dw_project(_nhwc(x).to(DEV), wd.reshape(hid, 9).t().contiguous().to(DEV), bd.to(DEV), wpp, bpp,
                 out, B=B, IH=H, IW=H, hid=hid, Cout=cout, OH=OH, OW=OW, stride=stride, dil=dil,
                 res=None if r is None else _nhwc(r).to(DEV))
    torch.cuda.synchronize()
    assert _rel(_nchw(out).cpu(), ref) < 1e-2
    _, bound = BC.dw_project_bound(x, wd, bd, wp.to(torch.bfloat16), bp, stride=stride, dil=dil, res=r)
    _within(_nchw(out), bound, "dw_project")
    assert _guards_kept(raw, 7.0)


@pytest.mark.parametrize("hid,cout,stride,dil,res", BC.DW_PROJ_FUSED)
@pytest.mark.parametrize("waves,rows,stages,xcd", [(4, 0, 2, False), (8, 0, 2, False), (4, 2, 2, False),
                                                   (4, 3, 2, False), (4, 3, 3, True), (4, 2, 4, True),
                                                   (4, 6, 3, True)])
def test_dw_proj_fused(hid, cout, stride, dil, res, waves, rows, stages, xcd):
    """Weight-streamed depthwise + projection (dw_proj.hip) vs the torch composition."""
    K = _hip()
    if rows and stride != 1:
        pytest.skip("row tiles: stride 1 only")
    g = torch.Generator().manual_seed(11)
    B, H = 3, 19
    x = F.relu6(torch.randn(B, hid, H, H, generator=g) * 2).to(torch.bfloat16)
    wd = torch.randn(hid, 1, 3, 3, generator=g) / 3
    bd = torch.randn(hid, generator=g) * 0.1
    wp = (torch.randn(cout, hid, generator=g) / hid ** 0.5).to(torch.bfloat16)
    bp = torch.randn(cout, generator=g) * 0.1
    d = F.relu6(F.conv2d(x.float(), wd, bd, stride, dil, dil, groups=hid)).to(torch.bfloat16).float()
    ref = F.conv2d(d, wp.float()[:, :, None, None], bp)
    OH, OW = ref.shape[-2:]
    r = torch.randn(B, cout, OH, OW, generator=g).to(torch.bfloat16) if res else None
    if res:
        ref = ref + r.float()
    wpk = K.pack_dw_proj(wp.to(DEV), wd.reshape(hid, 9).t().contiguous().to(DEV), bd.to(DEV))
    raw, out = _guarded_out((B, OH, OW, cout), float("nan"))
    K.dw_proj_fused(_nhwc(x).to(DEV).half(), wpk, bp.to(DEV), out, B=B, IH=H, IW=H, hid=hid, Cout=cout,
                    OH=OH, OW=OW, stride=stride, dil=dil, res=None if r is None else _nhwc(r).to(DEV),
                    waves=waves, rows=rows, stages=stages, xcd=xcd)
    torch.cuda.synchronize()
    assert torch.isfinite(out).all()
    assert _rel(_nchw(out).cpu(), ref) < 2e-2  # fp16 depthwise: rounding differs from bf16
    bound = _bound(("dw_proj_fused", hid, cout, stride, dil, res), lambda: BC.dw_proj_fused_bound(
        x, wd, bd, wp, bp, stride=stride, dil=dil, res=r))
    _within(_nchw(out), bound, f"dw_proj_fused waves {waves} rows {rows} stages {stages}")
    assert _guards_kept(raw, float("nan"))


def test_pw_conv_fp16_out():
    K = _hip()
    g = torch.Generator().manual_seed(12)
    M, Cin, Cout = BC.PW_FP16
    x = (torch.randn(M, Cin, generator=g) * 0.5).to(torch.bfloat16)
    w = (torch.randn(Cout, Cin, generator=g) / Cin ** 0.5).to(torch.bfloat16)
    b = torch.randn(Cout, generator=g)
    ref = F.relu6(x.float() @ w.float().t() + b)
    raw, out = _guarded_out((M, Cout), 7.0, torch.float16)
    K.pw_conv(x.to(DEV), K.pack_pw_weights(w.to(DEV), b.to(DEV)), out, M=M, K=Cin, N=Cout,
              act="relu6", mt=2, nch=3)
    torch.cuda.synchronize()
    assert _rel(out.float().cpu(), ref) < 2e-3
    _within(out, BC.mat_bound(x, w, b, act="relu6", fmt="fp16"), "pw_conv fp16 out")  # u = 2^-11
    assert _guards_kept(raw, 7.0)


@pytest.mark.parametrize("variant", [1, 2, 3, 4, 7, 8, 12, 13, 18, 19, 20])
@pytest.mark.parametrize("Cin,Cout,k,stride,dil,res,mode", [
    (64, 256, 1, 1, 1, True, "i8"), (256, 64, 3, 2, 1, False, "i8"), (512, 512, 3, 1, 2, False, "i8"),
    (256, 19, 1, 1, 1, False, "bf16"), (1024, 256, 1, 1, 1, False, "i8"), (208, 136, 3, 1, 3, True, "i8")])
def test_conv_i8(Cin, Cout, k, stride, dil, res, mode, variant):
    K = _hip()
    g = torch.Generator().manual_seed(12)
    B, H = 2, 17
    x8 = torch.randint(-127, 128, (B, Cin, H, H), generator=g, dtype=torch.int32)
    w8 = torch.randint(-127, 128, (Cout, Cin, k, k), generator=g, dtype=torch.int32)
    # accumulators have a standard deviation of 5376 sqrt(Cin k^2) (5376: that of a product of
    # two uniform +-127 codes): ~40 output steps of 0.05 after scaling, so the codes stay interior
    sc = (0.5 + torch.rand(Cout, generator=g)) * 0.05 * 40 / (5376 * (Cin * k * k) ** 0.5)
    bi = torch.randn(Cout, generator=g) * 10 * 0.05
    acc = F.conv2d(x8.double(), w8.double(), None, stride, dil * (k // 2), dil)  # exact
    ref = acc.float() * sc.view(1, -1, 1, 1) + bi.view(1, -1, 1, 1)
    OH, OW = ref.shape[-2:]
    r8 = None
    if res:
        r8 = torch.randint(-127, 128, (B, Cout, OH, OW), generator=g, dtype=torch.int32)
        ref = ref + r8.float() * 0.02
    ref = torch.relu(ref)
    xin = _nhwc(x8.to(torch.int8)).to(DEV)
    wk = w8.to(torch.int8).permute(0, 2, 3, 1).contiguous().to(DEV)
    if mode == "i8":
        out = torch.empty(B, OH, OW, Cout, dtype=torch.int8, device=DEV)
        K.conv_i8(xin, wk, sc.to(DEV), bi.to(DEV), out, B=B, IH=H, IW=H, Cin=Cin, OH=OH, OW=OW,
                  Cout=Cout, k=k, stride=stride, dil=dil, act="relu",
                  res=None if r8 is None else _nhwc(r8.to(torch.int8)).to(DEV), res_scale=0.02,
                  out_scale=0.05, variant=variant)
        torch.cuda.synchronize()
        exp = torch.clamp(torch.round(ref / 0.05), -127, 127)
        sat = (exp.abs() == 127).float().mean().item()
        assert sat <= 0.05 and (exp > 0).float().mean() > 0.3, sat  # an error is not hidden by the clamp
        diff = (_nchw(out).cpu().float() - exp).abs()
        assert diff.max() <= 1 and (diff > 0).float().mean() < 1e-3
    else:
        out = torch.empty(B, OH, OW, Cout, dtype=torch.bfloat16, device=DEV)
        K.conv_i8(xin, wk, sc.to(DEV), bi.to(DEV), out, B=B, IH=H, IW=H, Cin=Cin, OH=OH, OW=OW,
                  Cout=Cout, k=k, stride=stride, dil=dil, act="relu", variant=variant)
        torch.cuda.synchronize()
        assert _rel(_nchw(out).cpu(), ref) < 5e-3


# (Cout, ldo, co_off, output): every store path of the conv_i8 epilogues
_I8_LAYOUTS = [(64, 192, 64, "i8"),    # aligned 16-byte stores into a channel slice
               (64, 200, 72, "i8"),    # slice at an 8-byte offset: the byte-store fallback
               (40, 40, 0, "i8"),      # channel tail (40 = 2 x 16 + 8)
               (19, 24, 0, "bf16"),    # the logits row: 19 channels in a row of 24
               (21, 24, 0, "bf16"),
               (64, 68, 4, "bf16")]    # bf16 slice that no 16-byte store reaches


def _i8_epilogue_case(k, dil, Cout, seed):
    """Operands of the epilogue test, scaled so the codes stay interior: accumulators have a
    standard deviation of 5376 sqrt(Cin k^2) (5376: that of a product of two uniform +-127
    codes), so scale = u * out_scale * 40 / that puts ~40 output steps on them; bias and the
    per-image bias ~ N(0, (10 steps)^2), the residual adds 0.3 steps per code."""
    g = torch.Generator().manual_seed(seed)
    B, H, Cin, out_scale = 2, 13, 128, 0.05
    x8 = torch.randint(-127, 128, (B, Cin, H, H), generator=g, dtype=torch.int32)
    w8 = torch.randint(-127, 128, (Cout, Cin, k, k), generator=g, dtype=torch.int32)
    sc = (0.5 + torch.rand(Cout, generator=g)) * out_scale * 40 / (5376 * (Cin * k * k) ** 0.5)
    bi = torch.randn(Cout, generator=g) * 10 * out_scale
    ib = torch.randn(B, Cout, generator=g) * 10 * out_scale
    r8 = torch.randint(-127, 128, (B, Cout, H, H), generator=g, dtype=torch.int32)
    return dict(B=B, H=H, Cin=Cin, out_scale=out_scale, res_scale=0.3 * out_scale, x8=x8, w8=w8, sc=sc,
                bi=bi, ib=ib, r8=r8)


@pytest.mark.parametrize("Cout,ldo,co_off,mode", _I8_LAYOUTS)
@pytest.mark.parametrize("k,dil", [(1, 1), (3, 5)])
def test_conv_i8_epilogue(k, dil, Cout, ldo, co_off, mode):
    """Every ``conv_i8`` variant against a float64 reference computed on the CPU (never
    against another variant), over the epilogue's branches: act None / relu / relu6, with and
    without a per-image bias, with and without an int8 residual, into every output layout.
    B = 2, 13 x 13 (M = 338: partial tiles that straddle the image boundary), Cin = 128.
    int8: at most one step off on <= 1e-3 of the codes; bf16: 2^-8 relative + 1e-6 elementwise.
    The neighbours of a channel slice and the padding of a row keep their sentinel. With
    act None the codes reach -127 and never -128, in the reference and in the output. The
    saturated share of the reference is asserted <= 5 % (measured on the CPU: <= 1.5 %)."""
    import int8_ref as I
    from semantic_segmentation_server_amd.models.hip_int8 import _I8_VARIANTS
    K = _hip()
    c = _i8_epilogue_case(k, dil, Cout, seed=41 + k)
    B, H, Cin, s_out = c["B"], c["H"], c["Cin"], c["out_scale"]
    i8 = mode == "i8"
    variants = list(_I8_VARIANTS) + [12, 13]
    if K.conv_i8_1x1_ok(Cin=Cin, Cout=Cout, k=k, ldo=ldo, co_off=co_off, int8_out=i8):
        variants += [5, 6, 10, 11]
    xin = _nhwc(c["x8"].to(torch.int8)).to(DEV)
    wk = c["w8"].to(torch.int8).permute(0, 2, 3, 1).contiguous().to(DEV)
    sc, bi, ib = c["sc"].to(DEV), c["bi"].to(DEV), c["ib"].to(DEV)
    rin = _nhwc(c["r8"].to(torch.int8)).to(DEV)
    sentinel = 99 if i8 else float("nan")
    worst = (0.0, 0)
    for act in (None, "relu", "relu6"):
        for img in (False, True):
            for res in (False, True):
                v = I.exact_conv(c["x8"], c["w8"], c["sc"], c["bi"], 1.0, dil=dil,
                                 res_codes=c["r8"] if res else None, s_res=c["res_scale"],
                                 img_bias=c["ib"] if img else None, act=act)
                ref = I.requant(v, s_out) if i8 else v
                if i8:
                    assert I.saturated_share(ref) <= 0.05, (act, img, res, I.saturated_share(ref))
                    assert int(ref.min()) == (-127 if act is None else 0)
                    if act == "relu6":
                        assert int(ref.max()) == 120  # 6 / 0.05: the relu6 cap is live
                for variant in variants:
                    what = f"variant {variant} act {act} img_bias {img} res {res}"
                    out = torch.full((B, H, H, ldo), sentinel, dtype=torch.int8 if i8 else torch.bfloat16,
                                     device=DEV)
                    K.conv_i8(xin, wk, sc, bi, out, B=B, IH=H, IW=H, Cin=Cin, OH=H, OW=H, Cout=Cout, k=k,
                              dil=dil, ldo=ldo, co_off=co_off, act=act, res=rin if res else None,
                              res_scale=c["res_scale"], img_bias=ib if img else None,
                              out_scale=s_out if i8 else None, variant=variant)
                    torch.cuda.synchronize()
                    o = out.cpu()
                    got = _nchw(o[..., co_off:co_off + Cout])
                    rest = torch.cat([o[..., :co_off], o[..., co_off + Cout:]], -1)
                    if i8:
                        assert bool((rest == 99).all()), what + ": wrote outside its channel slice"
                        share, mx = I.assert_codes_close(got, ref, what)
                        worst = max(worst, (share, mx))
                        if act is None:
                            assert int(got.min()) == -127, what
                    else:
                        assert bool(torch.isnan(rest.float()).all()), what + ": wrote outside its channel slice"
                        I.assert_bf16_close(got, ref, what)
    print(f"conv_i8 epilogue k={k} {(Cout, ldo, co_off, mode)}: {len(variants)} variants, worst mismatch "
          f"share {worst[0]:.2e}, max step {worst[1]}")


@pytest.mark.parametrize("variant", [7, 2, 4, 8])
def test_conv_i8_epilogue_tap_group_perm(variant):
    """The 3x3 dilation-5 case of ``test_conv_i8_epilogue`` with the rows permuted into
    tap-uniform tiles (``tap_group_perm``), against the same float64 reference."""
    import int8_ref as I
    K = _hip()
    k, dil, Cout, ldo, co_off = 3, 5, 64, 192, 64
    c = _i8_epilogue_case(k, dil, Cout, seed=41 + k)
    B, H, Cin, s_out = c["B"], c["H"], c["Cin"], c["out_scale"]
    v = I.exact_conv(c["x8"], c["w8"], c["sc"], c["bi"], 1.0, dil=dil, res_codes=c["r8"],
                     s_res=c["res_scale"], img_bias=c["ib"], act="relu")
    ref = I.requant(v, s_out)
    assert I.saturated_share(ref) <= 0.05
    perm = K.tap_group_perm(B, H, H, 3, dil, K.I8_TILE[variant][0], device=DEV)
    assert perm.numel() > B * H * H  # more than one tap class: padded tiles
    out = torch.full((B, H, H, ldo), 99, dtype=torch.int8, device=DEV)
    K.conv_i8(_nhwc(c["x8"].to(torch.int8)).to(DEV), c["w8"].to(torch.int8).permute(0, 2, 3, 1).contiguous().to(DEV),
              c["sc"].to(DEV), c["bi"].to(DEV), out, B=B, IH=H, IW=H, Cin=Cin, OH=H, OW=H, Cout=Cout, k=k,
              dil=dil, ldo=ldo, co_off=co_off, act="relu", res=_nhwc(c["r8"].to(torch.int8)).to(DEV),
              res_scale=c["res_scale"], img_bias=c["ib"].to(DEV), out_scale=s_out, variant=variant, perm=perm)
    torch.cuda.synchronize()
    o = out.cpu()
    assert bool((o[..., :co_off] == 99).all()) and bool((o[..., co_off + Cout:] == 99).all())
    I.assert_codes_close(_nchw(o[..., co_off:co_off + Cout]), ref, f"variant {variant} with perm")


@pytest.mark.parametrize("IH,IW,C", [(65, 65, 64), (12, 9, 16), (1, 7, 32)])
def test_maxpool_i8(IH, IW, C):
    """``maxpool3x3s2_i8`` on codes over the whole -128..127 range, bit-equal to
    ``F.max_pool2d(x, 3, 2, 1)``: the padding never wins, not even over a window that holds
    only -128 (the first and the last window of image 0 do)."""
    K = _hip()
    g = torch.Generator().manual_seed(51)
    B = 2
    x = torch.randint(-128, 128, (B, C, IH, IW), generator=g, dtype=torch.int32)
    x[0, :, :2, :2] = -128  # all-negative windows at two borders
    x[0, :, -2:, -2:] = -128
    x[1, :, :2, :2] = torch.randint(-128, -100, (C, min(2, IH), 2), generator=g, dtype=torch.int32)
    ref = F.max_pool2d(x.float(), 3, 2, 1)
    OH, OW = ref.shape[-2:]
    assert ref[0, :, 0, 0].max() == -128 and ref.min() == -128 and ref.max() == 127
    out = torch.full((B, OH, OW, C), 99, dtype=torch.int8, device=DEV)
    K.maxpool3x3s2_i8(_nhwc(x.to(torch.int8)).to(DEV), out, B=B, IH=IH, IW=IW, C=C, OH=OH, OW=OW)
    torch.cuda.synchronize()
    assert torch.equal(_nchw(out).cpu().float(), ref)


def test_conv_i8_k64_rows_bit_identical():
    """64-byte K rows per LDS stage (variants 18-20) compute the same exact int32 sums and
    the same epilogue as the 128-byte form of the same tile (2 / 3 / 4): byte-identical."""
    K = _hip()
    g = torch.Generator().manual_seed(37)
    B, H = 2, 21
    for Cin, Cout, k, dil in ((64, 256, 1, 1), (208, 512, 1, 1), (512, 256, 3, 2)):
        x = torch.randint(-127, 128, (B, H, H, Cin), generator=g, dtype=torch.int32).to(torch.int8).to(DEV)
        w = torch.randint(-127, 128, (Cout, k, k, Cin), generator=g, dtype=torch.int32).to(torch.int8).to(DEV)
        sc = (torch.rand(Cout, generator=g) * 1e-4).to(DEV)
        bi = torch.randn(Cout, generator=g).to(DEV)
        outs = {}
        for v in (2, 3, 4, 18, 19, 20):
            o = torch.full((B, H, H, Cout), 99, dtype=torch.int8, device=DEV)
            K.conv_i8(x, w, sc, bi, o, B=B, IH=H, IW=H, Cin=Cin, OH=H, OW=H, Cout=Cout, k=k, dil=dil,
                      act="relu", out_scale=0.05, variant=v)
            outs[v] = o
        torch.cuda.synchronize()
        for v, base in ((18, 2), (19, 3), (20, 4)):
            assert torch.equal(outs[v].cpu(), outs[base].cpu()), (Cin, k, v)


@pytest.mark.parametrize("variant", [7, 2, 8])
def test_conv_i8_grouped_aspp(variant):
    """The int8 ASPP branches (1x1 + three atrous 3x3, one input, channel slices of one concat
    buffer) in ONE grouped LDS-DMA launch with tap-class row permutations and the LPT tile
    order: byte-identical to the four separate raster-order launches (same exact int32 sums,
    same epilogue), and the separate launch of a permuted branch matches too."""
    K = _hip()
    g = torch.Generator().manual_seed(variant)
    B, H, Cin, A = 2, 19, 256, 64
    BM = K.I8_TILE[variant][0]
    x = torch.randint(-127, 128, (B, H, H, Cin), generator=g, dtype=torch.int32).to(torch.int8).to(DEV)
    convs = []
    for j, (k, d) in enumerate([(1, 1), (3, 2), (3, 5), (3, 7)]):
        w = torch.randint(-127, 128, (A, k, k, Cin), generator=g, dtype=torch.int32).to(torch.int8).to(DEV)
        convs.append(dict(x=x, w=w, scale=(torch.rand(A, generator=g) * 1e-4).to(DEV),
                          bias=torch.randn(A, generator=g).to(DEV), B=B, IH=H, IW=H, Cin=Cin, OH=H,
                          OW=H, Cout=A, k=k, dil=d, ldo=4 * A, co_off=j * A, act="relu", out_scale=0.05))
    ref = torch.zeros(B, H, H, 4 * A, dtype=torch.int8, device=DEV)
    for cv in convs:
        kw = {k: v for k, v in cv.items() if k not in ("x", "w", "scale", "bias")}
        K.conv_i8(cv["x"], cv["w"], cv["scale"], cv["bias"], ref, variant=variant, **kw)
    gc = []
    for cv in convs:
        cv = dict(cv, out=torch.full((B, H, H, 4 * A), 99, dtype=torch.int8, device=DEV))
        if cv["k"] > 1:
            cv["perm"] = K.tap_group_perm(B, H, H, 3, cv["dil"], BM, device=DEV)
        gc.append(cv)
    out = torch.full((B, H, H, 4 * A), 99, dtype=torch.int8, device=DEV)
    for cv in gc:
        cv["out"] = out
    order = K.grouped_tile_order_i8(gc, variant, device=DEV)
    K.conv_i8_grouped(gc, order, variant)
    one = torch.full_like(out, 99)
    cv = gc[3]
    kw = {k: v for k, v in cv.items() if k not in ("x", "w", "scale", "bias", "out")}
    K.conv_i8(cv["x"], cv["w"], cv["scale"], cv["bias"], one, variant=variant, **kw)
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), ref.cpu())
    assert torch.equal(one[..., 3 * A:].cpu(), ref[..., 3 * A:].cpu())
    assert (one[..., :3 * A] == 99).all()  # the permuted launch wrote only its own slice


@pytest.mark.parametrize("Cin,Cout,res,img,mode,M", [
    (64, 64, False, False, "i8", 2 * 33 * 33), (64, 256, True, False, "i8", 2 * 33 * 33 + 0),
    (256, 64, False, True, "i8", 3 * 17 * 19), (128, 512, True, False, "i8", 2 * 17 * 17),
    (256, 1024, True, False, "i8", 2 * 17 * 17), (512, 128, False, False, "bf16", 2 * 9 * 9),
    (1024, 256, False, False, "i8", 1000), (64, 128, False, True, "i8", 3 * 77)])
def test_conv_i8_1x1_stream_exact(Cin, Cout, res, img, mode, M):
    """The streaming 1x1 variants (5, 6) against the register-fed one (1): same int32 sums;
    bf16 outputs bit-identical, int8 outputs within one rounding step of the float epilogue
    (pixel tails, residual, per-image bias)."""
    K = _hip()
    g = torch.Generator().manual_seed(31)
    B = 3 if M % 3 == 0 else 1
    H, W = 1, M // B
    x8 = torch.randint(-127, 128, (B, H, W, Cin), generator=g, dtype=torch.int32).to(torch.int8).to(DEV)
    w8 = torch.randint(-127, 128, (Cout, Cin), generator=g, dtype=torch.int32).to(torch.int8).to(DEV)
    sc = (torch.rand(Cout, generator=g) * 1e-4).to(DEV)
    bi = torch.randn(Cout, generator=g).to(DEV)
    r8 = (torch.randint(-127, 128, (B, H, W, Cout), generator=g, dtype=torch.int32).to(torch.int8).to(DEV)
          if res else None)
    ib = torch.randn(B, Cout, generator=g).to(DEV) if img else None
    outs = []
    for v in (1, 5, 6, 10, 11):
        dt = torch.int8 if mode == "i8" else torch.bfloat16
        out = torch.zeros(B, H, W, Cout, dtype=dt, device=DEV)
        K.conv_i8(x8, w8, sc, bi, out, B=B, IH=H, IW=W, Cin=Cin, OH=H, OW=W, Cout=Cout, act="relu",
                  res=r8, res_scale=0.02, img_bias=ib, out_scale=0.05 if mode == "i8" else None, variant=v)
        outs.append(out)
    torch.cuda.synchronize()
    for o in outs[1:]:
        if mode == "bf16":  # the float epilogue, shared
            assert torch.equal(outs[0].cpu(), o.cpu())
        else:  # folded requantisation: at most one rounding step, rarely
            d = (outs[0].cpu().int() - o.cpu().int()).abs()
            assert d.max() <= 1 and (d > 0).float().mean() < 2e-3, (d.max(), (d > 0).float().mean())


def test_conv_i8_1x1_stride2_stream():
    """The streaming 1x1 variants on a strided projection shortcut (256 -> 512, stride 2)
    against the register-fed one: within one rounding step."""
    K = _hip()
    g = torch.Generator().manual_seed(35)
    B, H, Cin, Cout = 2, 17, 256, 512
    OH = (H - 1) // 2 + 1
    x8 = torch.randint(-127, 128, (B, H, H, Cin), generator=g, dtype=torch.int32).to(torch.int8).to(DEV)
    w8 = torch.randint(-127, 128, (Cout, Cin), generator=g, dtype=torch.int32).to(torch.int8).to(DEV)
    sc = (torch.rand(Cout, generator=g) * 1e-4).to(DEV)
    bi = torch.randn(Cout, generator=g).to(DEV)
    outs = []
    for v in (1, 5, 6, 10, 11):
        out = torch.zeros(B, OH, OH, Cout, dtype=torch.int8, device=DEV)
        K.conv_i8(x8, w8, sc, bi, out, B=B, IH=H, IW=H, Cin=Cin, OH=OH, OW=OH, Cout=Cout, k=1, stride=2,
                  act=None, out_scale=0.05, variant=v)
        outs.append(out)
    torch.cuda.synchronize()
    for o in outs[1:]:
        d = (outs[0].cpu().int() - o.cpu().int()).abs()
        assert d.max() <= 1 and (d > 0).float().mean() < 2e-3, (d.max(), (d > 0).float().mean())


@pytest.mark.parametrize("Cin,Cout,stride,dil,res", [(64, 64, 1, 1, False), (128, 128, 1, 1, True),
                                                    (128, 64, 2, 1, False), (64, 32, 1, 2, False),
                                                    (256, 256, 1, 2, False)])
def test_conv_i8_3x3_stream(Cin, Cout, stride, dil, res):
    """The streaming kernel's 3x3 form (taps as extra K fragments from shifted pixels, zero
    outside the image) against the register-fed variant: within one rounding step."""
    K = _hip()
    g = torch.Generator().manual_seed(33)
    B, H = 2, 19
    OH = (H - 1) // stride + 1
    x8 = torch.randint(-127, 128, (B, H, H, Cin), generator=g, dtype=torch.int32).to(torch.int8).to(DEV)
    w8 = torch.randint(-127, 128, (Cout, 3, 3, Cin), generator=g, dtype=torch.int32).to(torch.int8).to(DEV)
    sc = (torch.rand(Cout, generator=g) * 1e-5).to(DEV)
    bi = torch.randn(Cout, generator=g).to(DEV)
    r8 = (torch.randint(-127, 128, (B, OH, OH, Cout), generator=g, dtype=torch.int32).to(torch.int8).to(DEV)
          if res else None)
    outs = []
    for v in (1, 5, 6, 10, 11):
        out = torch.zeros(B, OH, OH, Cout, dtype=torch.int8, device=DEV)
        K.conv_i8(x8, w8, sc, bi, out, B=B, IH=H, IW=H, Cin=Cin, OH=OH, OW=OH, Cout=Cout, k=3, stride=stride,
                  dil=dil, act="relu", res=r8, res_scale=0.02, out_scale=0.05, variant=v)
        outs.append(out)
    torch.cuda.synchronize()
    for o in outs[1:]:
        d = (outs[0].cpu().int() - o.cpu().int()).abs()
        assert d.max() <= 1 and (d > 0).float().mean() < 2e-3, (d.max(), (d > 0).float().mean())


def test_int8_resnet50_matches_fake_quant():
    from semantic_segmentation_server_amd.models.deeplab import build_model
    from semantic_segmentation_server_amd.models.hip_int8 import HipDeepLabInt8
    from semantic_segmentation_server_amd.models.quant import fake_quant_forward
    from semantic_segmentation_server_amd.ops import reference_ops as R
    S = 129
    from semantic_segmentation_server_amd.models.quant import calibrate
    from semantic_segmentation_server_amd.runtime.sources import SyntheticSource
    model = build_model("resnet50", 19, calibrate_hw=65)
    lx, ly, *_ = R.letterbox_luts(160, 120, S, S)
    f, _, _ = SyntheticSource(160, 120, pool=2, seed=13).read_batch(2)
    frames = torch.from_numpy(f)
    x = R.preprocess(frames, lx, ly)
    scales = calibrate(model.float(), x)  # calibrate on the evaluation distribution
    hm = HipDeepLabInt8(model, torch.device(DEV), _small_cfg(arch="resnet50", dtype="int8"),
                        scales=scales)
    ref = fake_quant_forward(model.float(), hm.scales, x)
    with torch.no_grad():
        fp = model.float()(x)
    got = _nchw(hm.logits(frames.to(DEV), torch.tensor(lx, device=DEV),
                          torch.tensor(ly, device=DEV)).float()).cpu()
    e_fq, e_fp = _rel(got, ref), _rel(got, fp)
    print(f"int8 resnet50: rel err vs fake-quant {e_fq:.4f}, vs fp32 {e_fp:.4f}")
    assert e_fq < 0.03
    assert e_fp < 0.15
    agree = (got.argmax(1) == fp.argmax(1)).float().mean().item()
    assert agree > 0.95, agree


def test_int8_resnet50_headline_shape():
    """BASELINE config 4 as benchmarked: DeepLabv3-ResNet50 1025^2, B = 8, 2048x1024
    camera, the engine's own model / calibration and the COMMITTED plan
    (assets/tune_mi355x.json) -- the 160x128 LDS-DMA tiles, streaming 1x1 / 3x3 kernels
    at the grids that produce the bench number.

    Checked step by step with teacher forcing (tests/int8_ref.py ``check_plan``, the walker
    of tests/test_int8_plan.py on the picked variants): the int8 stem, the int8 max pool,
    every backbone conv, the ASPP branches and the projection against exact arithmetic on the
    plan's OWN input codes (at most one step off, on <= 1e-3 of the codes; the pool
    bit-equal), the pooled branch's per-image bias, the bf16 logits and the label map of the
    plan's own logits. End to end the random-init int8 network
    is chaotic -- a one-step rounding tie flipped in block 0 doubles its share of mismatched
    codes every block (scripts/int8_layer_diff.py: 2e-5 at block 0, 0.6 at block 15, with the
    stem modelled exactly) -- so the logits' distance to the fp32 fake-quant replay is bounded
    loosely, and reruns of the plan must be bit-identical."""
    import json
    from semantic_segmentation_server_amd import config as C
    from semantic_segmentation_server_amd.models.hip_model import TUNE_FILE_DEFAULT
    from semantic_segmentation_server_amd.models.quant import fake_quant_forward
    from semantic_segmentation_server_amd.ops import reference_ops as R
    from semantic_segmentation_server_amd.runtime.engine import Engine
    from semantic_segmentation_server_amd.runtime.sources import SyntheticSource
    B, S, cw, ch = 8, 1025, 2048, 1024
    key = f"resnet50_int8:B={B}:cam={cw}x{ch}:in={S}"
    saved = json.load(open(TUNE_FILE_DEFAULT))
    assert key in saved, "config 4 has no committed plan"
    cfg = C.Config(arch="resnet50", dtype="int8", input_size=S, batch=B, backend="hip", graph=False,
                   num_classes=19, dataset="cityscapes", camera_width=cw, camera_height=ch)
    eng = Engine(cfg, torch.device(DEV))
    eng.set_camera(cw, ch)
    hm = eng._hip_model
    f, _, _ = SyntheticSource(cw, ch, pool=4, seed=21).read_batch(B)
    frames = torch.from_numpy(np.ascontiguousarray(f)).to(DEV)
    got = hm.logits(frames, eng.lut_x, eng.lut_y).clone()
    bufs = {k: v.clone() for k, v in hm._plans[(B, ch, cw)][1].items()}
    again = hm.logits(frames, eng.lut_x, eng.lut_y)
    torch.cuda.synchronize()
    assert torch.equal(got, again), "int8 plan reruns differ"
    assert all(saved[key].get(n) == v for n, v in hm.choices.items() if n in saved[key]), \
        "the plan under test is not the committed one"
    # every step of the committed plan as this run left it (the picks only), each against exact
    # arithmetic on the step's own input buffers; the references stay on the device
    import int8_ref as I
    rep = I.check_plan(hm, hm._plans[(B, ch, cw)][0], bufs, frames, eng.lut_x, eng.lut_y, run=False,
                       ref_device=DEV, interior=False)
    assert len(rep) == 2 + 16 * 3 + 4 + 2, len(rep)  # stem, pool, 52 backbone convs, ASPP, projection
    print("teacher-forced per-step mismatch: worst " + str(I.worst(rep)))
    x = R.preprocess(frames.cpu(), eng.lut_x.cpu(), eng.lut_y.cpu()).to(DEV)
    import copy
    m32 = copy.deepcopy(eng.model).float().to(DEV)
    # the replay rounds the stem where the committed stem kernel does (bf16 MFMA or fp32)
    ref = fake_quant_forward(m32, hm.scales, x, stem_bf16=hm.choices["stem"] != "fp32").float()
    got = _nchw(got.float())
    e_fq = _rel(got.cpu(), ref.cpu())
    d_agree, frac = R.decisive_agreement(got, ref)
    print(f"int8 resnet50 1025^2 B={B}: rel err vs fake-quant {e_fq:.4f}; decisive pixels "
          f"({frac:.3f} of all) agreement {d_agree:.4f}")
    assert e_fq < 0.25, e_fq


def _records_equal(pa: torch.Tensor, pb: torch.Tensor) -> bool:
    """Packed records [F, 1 + 5K] equal in their valid part (slots past each frame's
    count are don't-care: they keep whatever an earlier frame left there)."""
    pa, pb = pa.cpu(), pb.cpu()
    if pa.shape != pb.shape or not torch.equal(pa[:, 0], pb[:, 0]):
        return False
    return all(torch.equal(pa[f, :1 + 5 * int(pa[f, 0])], pb[f, :1 + 5 * int(pb[f, 0])])
               for f in range(pa.shape[0]))


def test_stream_group_matches_single_engine(monkeypatch):
    # autotuning picks kernel variants per batch size (and variants round
    # differently); pin the choice so the two batchings run the same kernels
    monkeypatch.setenv("SSA_FUSED_IR", "1")
    from semantic_segmentation_server_amd.runtime.engine import Engine
    from semantic_segmentation_server_amd.runtime.multistream import StreamGroup
    from semantic_segmentation_server_amd.runtime.sources import SyntheticSource
    cfg = _small_cfg(graph=True, batch=4)
    grp = StreamGroup(cfg, torch.device(DEV), 2)
    one = Engine(cfg, torch.device(DEV))
    for e in (grp, one):
        e.set_camera(200, 150)
    f, _, _ = SyntheticSource(200, 150, pool=4).read_batch(4)
    d = torch.from_numpy(f).to(DEV)
    _, p1 = one.run_device(d)
    p1 = p1.clone()
    for _ in range(2):
        _, p2 = grp.run_device(d)
    torch.cuda.synchronize()
    assert _records_equal(p1, p2)
    # bound staging slots with split model / post-processing graphs per stream
    bufs = [torch.empty_like(d) for _ in range(2)]
    monkeypatch.setenv("GPU_MAX_HW_QUEUES", "8")  # 2 streams x 2 + 1 must fit for the split path
    grp.bind_inputs(bufs, split_post=True)
    assert grp.result_stream is not None
    for it in range(2):
        for b in bufs:
            b.copy_(d)
            torch.cuda.synchronize()
            _, p3 = grp.run_device(b)
            with torch.cuda.stream(grp.result_stream):
                p3 = p3.clone()
            torch.cuda.synchronize()
            assert _records_equal(p1, p3), it


@pytest.mark.parametrize("cin,cout,dil,H,S", BC.FUSED_IR_STREAM)
def test_fused_ir_stream(cin, cout, dil, H, S):
    """Wave-specialised fused IR kernel vs the fp32 torch block and vs the numpy
    re-execution of its data flow from the packed chunk images."""
    from semantic_segmentation_server_amd.ops import fused_span as FS
    from test_fused_span_cpu import _block, pack_block  # tests/ is on sys.path (prepend mode)
    W = 33
    if not FS.stream_supported(cin, cout, 1, H, W, S, dil):
        pytest.fail("shape expected to be supported")
    blk, spec = _block(cin, cout, dil, seed=cin * 5 + cout + dil)
    g = torch.Generator().manual_seed(23)
    B = 3
    x = torch.randn(B, cin, H, W, generator=g).to(torch.bfloat16)
    with torch.no_grad():
        ref = blk(x.float())
    packed = pack_block(blk, spec, device=DEV)
    table = FS.span_table(H, W, S, dil, DEV)
    xd = _nhwc(x).to(DEV)
    emu = FS.emulate_fused_span(_nhwc(x).float().numpy(), packed, table, residual=spec.residual)
    bound = BC.fused_ir_bound(x, dict(BC.unpack_fused_span(packed), dil=dil, residual=spec.residual), tile=True)
    variants = ((0, 1, 2) if cout <= 96 and dil == 1 else (0, 1)) + ((4,) if cout <= 160 else ()) + \
        ((6,) if cout <= 96 and dil == 1 else ())  # 4 / 6: the 3-slot chunk ring
    for variant in variants:
        out = torch.full((B, H, W, cout), float("nan"), dtype=torch.bfloat16, device=DEV)
        FS.fused_ir_stream(xd, packed, table, out, B=B, residual=spec.residual, variant=variant)
        torch.cuda.synchronize()
        assert torch.isfinite(out).all(), variant
        assert _rel(_nchw(out).cpu(), ref) < 2e-2, variant
        assert _rel(out.cpu().float(), torch.from_numpy(emu)) < 5e-3, variant
        _within(_nchw(out), bound, f"fused_ir_stream variant {variant}")
        # bit-exact rerun (no read of bytes another run or wave left behind)
        out2 = torch.full_like(out, float("nan"))
        FS.fused_ir_stream(xd, packed, table, out2, B=B, residual=spec.residual, variant=variant)
        torch.cuda.synchronize()
        assert torch.equal(out.view(torch.int16), out2.view(torch.int16)), variant
    # hidden split (batch-1 plans): the span's chunks over hs workgroups + stream_combine;
    # uneven chunk ranges (hs = 4 over 5 / 9 / 15 / 18 / 30 chunks) included
    nc = packed["hidP"] // 32
    for hs in (2, 4, nc):
        part = torch.full((hs * B * H * W * cout,), float("nan"), dtype=torch.float32, device=DEV)
        out = torch.full((B, H, W, cout), float("nan"), dtype=torch.bfloat16, device=DEV)
        FS.fused_ir_stream(xd, packed, table, out, B=B, residual=spec.residual, hsplit=hs, part=part)
        torch.cuda.synchronize()
        assert torch.isfinite(out).all(), hs
        assert _rel(_nchw(out).cpu(), ref) < 2e-2, hs
        assert _rel(out.cpu().float(), torch.from_numpy(emu)) < 5e-3, hs
        _within(_nchw(out), bound, f"fused_ir_stream hidden split {hs}")  # fp32 partials, stream_combine
        out2 = torch.full_like(out, float("nan"))
        FS.fused_ir_stream(xd, packed, table, out2, B=B, residual=spec.residual, hsplit=hs, part=part)
        torch.cuda.synchronize()
        assert torch.equal(out.view(torch.int16), out2.view(torch.int16)), hs
        # in-launch combine (each span's last arriving workgroup sums the slabs): the same
        # fixed-order arithmetic as stream_combine, so bit-identical; the tickets come back
        # zeroed, so repeated launches (graph replays) agree too
        cnt = torch.zeros(B * S, dtype=torch.int32, device=DEV)
        for rep in range(3):
            out3 = torch.full_like(out, float("nan"))
            FS.fused_ir_stream(xd, packed, table, out3, B=B, residual=spec.residual, hsplit=hs, part=part,
                               cnt=cnt)
            torch.cuda.synchronize()
            assert torch.equal(out.view(torch.int16), out3.view(torch.int16)), (hs, rep)
            assert int(cnt.abs().sum()) == 0, (hs, rep)


@pytest.mark.gpu
@pytest.mark.parametrize("cout,H,S", BC.FUSED_IR_LATTICE)
def test_fused_ir_stream_lattice(cout, H, S):
    """Dilation-2 blocks on lattice spans (variant bit 8): vs the fp32 torch block, vs the
    numpy re-execution of the lattice data flow, and bit-identical to the raster-span
    kernel (same fp16 depthwise chain per pixel, same fp32 projection order); the hidden
    split (stream_combine and in-launch combine) writes the same bytes."""
    from semantic_segmentation_server_amd.ops import fused_span as FS
    from test_fused_span_cpu import _block, pack_block
    cin, dil, W = 160, 2, 33
    assert FS.stream_supported(cin, cout, 1, H, W, S, dil, lattice=True)
    blk, spec = _block(cin, cout, dil, seed=cin * 3 + cout + H)
    g = torch.Generator().manual_seed(29)
    B = 3
    x = torch.randn(B, cin, H, W, generator=g).to(torch.bfloat16)
    with torch.no_grad():
        ref = blk(x.float())
    packed = pack_block(blk, spec, device=DEV)
    lt = FS.lattice_table(H, W, S, dil, DEV)
    rt = FS.span_table(H, W, S, dil, DEV)
    xd = _nhwc(x).to(DEV)
    emu = FS.emulate_fused_span(_nhwc(x).float().numpy(), packed, lt, residual=spec.residual)
    bound = BC.fused_ir_bound(x, dict(BC.unpack_fused_span(packed), dil=dil, residual=spec.residual), tile=True)
    raster = torch.full((B, H, W, cout), float("nan"), dtype=torch.bfloat16, device=DEV)
    FS.fused_ir_stream(xd, packed, rt, raster, B=B, residual=spec.residual, variant=1)
    for variant in ((0, 1, 2, 4) if cout <= 160 else (1,)):
        out = torch.full((B, H, W, cout), float("nan"), dtype=torch.bfloat16, device=DEV)
        FS.fused_ir_stream(xd, packed, lt, out, B=B, residual=spec.residual, variant=variant)
        torch.cuda.synchronize()
        assert torch.isfinite(out).all(), variant
        assert _rel(_nchw(out).cpu(), ref) < 2e-2, variant
        assert _rel(out.cpu().float(), torch.from_numpy(emu)) < 5e-3, variant
        _within(_nchw(out), bound, f"fused_ir_stream lattice variant {variant}")
        assert torch.equal(out.view(torch.int16), raster.view(torch.int16)), variant
    nc = packed["hidP"] // 32
    v = 0 if cout <= 160 else 1
    for hs in (2, 4):
        part = torch.full((hs * B * H * W * cout,), float("nan"), dtype=torch.float32, device=DEV)
        out = torch.full((B, H, W, cout), float("nan"), dtype=torch.bfloat16, device=DEV)
        FS.fused_ir_stream(xd, packed, lt, out, B=B, residual=spec.residual, variant=v, hsplit=hs, part=part)
        torch.cuda.synchronize()
        assert torch.isfinite(out).all(), hs
        assert _rel(_nchw(out).cpu(), ref) < 2e-2, hs
        _within(_nchw(out), bound, f"fused_ir_stream lattice hidden split {hs}")
        cnt = torch.zeros(B * S, dtype=torch.int32, device=DEV)
        out3 = torch.full_like(out, float("nan"))
        FS.fused_ir_stream(xd, packed, lt, out3, B=B, residual=spec.residual, variant=v, hsplit=hs, part=part,
                           cnt=cnt)
        torch.cuda.synchronize()
        assert torch.equal(out.view(torch.int16), out3.view(torch.int16)), hs
        assert int(cnt.abs().sum()) == 0, hs
    assert nc >= 4


@pytest.mark.parametrize("M,HW,ncls,ldo,img", BC.ASPP_HEAD)
@pytest.mark.parametrize("G", [None, 1, 2, 3, 5, 9])
@pytest.mark.parametrize("waves", [8, 16])
def test_aspp_head(M, HW, ncls, ldo, img, G, waves):
    """Fused ASPP projection + logits vs fp32 torch: relu(cat Wp^T + bp + ib) rounded to
    bf16 (the kernel's on-chip projection tile), then Wl . proj + bl."""
    K = _hip()
    g = torch.Generator().manual_seed(11)
    Kd = 1024
    cat = torch.relu(torch.randn(M, Kd, generator=g)).to(torch.bfloat16)
    wp = (torch.randn(256, Kd, generator=g) / Kd ** 0.5).to(torch.bfloat16)
    bp = torch.randn(256, generator=g) * 0.1
    wl = (torch.randn(ncls, 256, generator=g) / 16).to(torch.bfloat16)
    bl = torch.randn(ncls, generator=g)
    ib = torch.randn(M // HW, 256, generator=g) * 0.5 if img else None
    proj = cat.float() @ wp.float().t() + bp
    if img:
        proj = proj + ib.repeat_interleave(HW, 0)
    proj = torch.relu(proj).to(torch.bfloat16).float()
    ref = proj @ wl.float().t() + bl
    packed = K.pack_aspp_head(wp, bp, wl, bl, device=DEV)
    raw, out = _guarded_out((M, ldo), float("nan"))  # rows past M: the last pixel group is partial
    K.aspp_head(cat.to(DEV), packed, out, M=M, HW=HW, ldo=ldo,
                img_bias=None if ib is None else ib.to(DEV), G=G, waves=waves)
    torch.cuda.synchronize()
    got = out.float().cpu()
    assert torch.isfinite(got).all()
    assert _rel(got[:, :ncls], ref) < 1e-2
    assert torch.all(got[:, ncls:] == 0)
    bound = _bound(("aspp_head", M, HW, ncls, img), lambda: BC.aspp_head_bound(
        cat, wp, bp, wl, bl, None if ib is None else ib.repeat_interleave(HW, 0)))
    _within(got[:, :ncls], bound, f"aspp_head G {G} waves {waves}")
    assert _guards_kept(raw, float("nan"))


@pytest.mark.parametrize("cin,cout,stride,H,W", BC.FUSED_IR_BAND)
@pytest.mark.parametrize("R,nslot", [(8, 2), (5, 1), (3, 2)])
def test_fused_ir_band(cin, cout, stride, H, W, R, nslot):
    """Row-streaming fused block vs the fp32 torch block, and vs the numpy re-execution
    of its own data flow from the packed blob."""
    from semantic_segmentation_server_amd.ops import fused_band as FB
    from test_fused_band_cpu import band_block, pack_band  # tests/ is on sys.path
    blk, spec = band_block(cin, cout, stride, seed=cin * 5 + cout + stride)
    g = torch.Generator().manual_seed(31)
    B = 2
    x = torch.randn(B, cin, H, W, generator=g).to(torch.bfloat16)
    with torch.no_grad():
        ref = blk(x.float())
    packed = pack_band(blk, spec, device=DEV)
    if FB.band_lds(packed, stride, (W - 1) // stride + 1, nslot) > 160 * 1024:
        pytest.skip("LDS")
    assert FB.band_supported(cin, spec.hidden, cout, stride, 1, (W - 1) // stride + 1)
    OH, OW = (H - 1) // stride + 1, (W - 1) // stride + 1
    emu = bound = None
    # hs 2: two waves per column group; split 2: two column bands (blocks 1-2)
    cfgs = [(hs, sp) for sp in (1, 2) for hs in (1, 2)
            if FB.band_supported(cin, spec.hidden, cout, stride, 1, OW, sp) and FB.band_waves(OW, sp) <= (8 if hs == 2 else 99)]
    for hs, sp in cfgs:
        if FB.band_lds(packed, stride, OW, nslot, hs, sp) > 160 * 1024:
            continue
        out = torch.full((B, OH, OW, cout), float("nan"), dtype=torch.bfloat16, device=DEV)
        FB.fused_ir_band(_nhwc(x).to(DEV), packed, out, B=B, IH=H, IW=W, stride=stride,
                         residual=spec.residual, R=R, nslot=nslot, hs=hs, split=sp)
        torch.cuda.synchronize()
        assert torch.isfinite(out).all(), (hs, sp)
        assert _rel(_nchw(out).cpu(), ref) < 2e-2, (hs, sp)
        # the weights are drawn from the global generator: one reference per test, not per shape
        bound = bound or BC.fused_ir_bound(x, BC.unpack_fused_band(packed, stride, spec.residual), tile=True)
        _within(_nchw(out), bound, f"fused_ir_band R {R} nslot {nslot} hs {hs} split {sp}")
        if H * W <= 129 * 129:
            if emu is None:
                emu = FB.emulate_fused_band(_nhwc(x).float().numpy(), packed, stride=stride,
                                            residual=spec.residual)
            assert _rel(out.cpu().float(), torch.from_numpy(emu)) < 5e-3, (hs, sp)


@pytest.mark.parametrize("cin,cout,stride,H,W", BC.FUSED_IR_BAND)
@pytest.mark.parametrize("R", [8, 5, 17])
def test_fused_ir_slice(cin, cout, stride, H, W, R):
    """Hidden-sliced row-streaming block (one wave per column group x hidden chunk, the
    chunk's weights in VGPRs): vs the fp32 torch block, and bit-identical to the band
    kernel (same blob, same accumulation order) at every instantiated width."""
    from semantic_segmentation_server_amd.ops import fused_band as FB
    from test_fused_band_cpu import band_block, pack_band  # tests/ is on sys.path
    blk, spec = band_block(cin, cout, stride, seed=cin * 5 + cout + stride)
    g = torch.Generator().manual_seed(37)
    B = 2
    x = torch.randn(B, cin, H, W, generator=g).to(torch.bfloat16)
    with torch.no_grad():
        ref = blk(x.float())
    packed = pack_band(blk, spec, device=DEV)
    OH, OW = (H - 1) // stride + 1, (W - 1) // stride + 1
    widths = FB.slice_widths(cin, spec.hidden, cout, stride, 1)
    assert widths
    xd = _nhwc(x).to(DEV)
    band = None
    if FB.band_supported(cin, spec.hidden, cout, stride, 1, OW):
        band = torch.full((B, OH, OW, cout), float("nan"), dtype=torch.bfloat16, device=DEV)
        FB.fused_ir_band(xd, packed, band, B=B, IH=H, IW=W, stride=stride, residual=spec.residual,
                         R=R, nslot=2)
    first = None
    for nw in widths:
        for oneb in (False, True):  # one barrier per input row: same arithmetic, bit-identical
            if FB.slice_lds(packed, stride, OW, nw, oneb) > 160 * 1024:
                continue
            out = torch.full((B, OH, OW, cout), float("nan"), dtype=torch.bfloat16, device=DEV)
            FB.fused_ir_slice(xd, packed, out, B=B, IH=H, IW=W, stride=stride, residual=spec.residual,
                              R=R, nw=nw, one_barrier=oneb)
            torch.cuda.synchronize()
            assert torch.isfinite(out).all(), (nw, oneb)
            assert _rel(_nchw(out).cpu(), ref) < 2e-2, (nw, oneb)
            if first is None:  # every later output must equal this one bit for bit
                _within(_nchw(out), BC.fused_ir_bound(x, BC.unpack_fused_band(packed, stride, spec.residual),
                                                      tile=True), f"fused_ir_slice R {R} nw {nw}")
            if band is not None:
                assert torch.equal(out, band), (nw, oneb, (out.float() - band.float()).abs().max().item())
            if first is None:
                first = out
            assert torch.equal(out, first), (nw, oneb)


def test_multistream_batched_step_tags_streams():
    """Config 5 as one batched step: 4 camera streams x 2 frames fill one 8-frame graph
    replay; every record lands in its own stream's hub buffer (v2 per-stream reads) with a
    frame id of that stream, and the records equal the plain engine step's."""
    from semantic_segmentation_server_amd.parallel import dist as D
    from semantic_segmentation_server_amd.parallel.dp import DataParallelPipeline
    from semantic_segmentation_server_amd.runtime.engine import Engine
    from semantic_segmentation_server_amd.runtime.results import ResultHub
    from semantic_segmentation_server_amd.runtime.sources import SyntheticSource
    S, per = 4, 2
    B = S * per
    eng = Engine(_small_cfg(graph=True, batch=B, input_size=257, min_area_ratio=0.002),
                 torch.device(DEV))
    src = SyntheticSource(160, 120, seed=7, pool=8)
    frames = torch.from_numpy(np.ascontiguousarray(src.read_batch(B)[0]))
    eng.set_camera(160, 120)
    fids = list(range(100, 100 + B))
    streams = [i % S for i in range(B)]  # round-robin, as the feeder interleaves cameras
    _, post = eng._step_device(frames.to(DEV))
    want = eng._hip_post.fetch(post, fids, [0.0] * B, streams, eng.W, eng.H)
    torch.cuda.synchronize()
    assert len(want) > 0
    hub = ResultHub(S, maxlen=10000)
    pipe = DataParallelPipeline(D.init(), eng, 160, 120, B, "local", hub, S, lag=1)
    pipe.prefetch(frames.pin_memory())
    pipe.step(frame_ids=fids, ts=[0.0] * B, streams=streams)
    pipe.flush()
    torch.cuda.synchronize()
    total = 0
    for s in range(S):
        got = hub.get(s).pop(10000) if hub.get(s) is not None else []
        exp = want[want["stream"] == s]
        assert sorted((int(r["frame"]), int(r["label"])) for r in got) == \
            sorted((int(f), int(l)) for f, l in zip(exp["frame"], exp["label"])), s
        assert all(int(r["frame"]) % S == (100 + s) % S for r in got)
        total += len(got)
    assert total == len(want)
