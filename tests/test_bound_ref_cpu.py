"""The error-bounded float64 references (tests/bound_ref.py, tests/bound_cases.py) judged on
the CPU, at the exact shapes the device tests use.

Soundness: a torch emulation of a correct kernel (fp32 accumulation, rounding at the stated
points) lies inside the bound at every element, in two accumulation orders: the whole conv,
and the sum of per-tap (k > 1) or per-Cin-chunk (k = 1) partial convs.

Teeth: one wrong element is rejected. The mutated site is chosen deterministically as the
first one in raster order at which the mutation changes the stored value and no rounding
flip is possible (e = 0), so a coincidence (equal neighbours after a ReLU) cannot excuse it.
"""
import pytest
import torch
import torch.nn.functional as F

import bound_cases as C
import bound_ref as BR

ORDERS = ["whole", "parts"]


# ---------------------------------------------------------------- the rounding stage itself
@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
def test_rnd_is_the_formats_cast(fmt):
    g = torch.Generator().manual_seed(0)
    x = torch.randn(200000, generator=g) * torch.exp2(torch.randint(-20, 8, (200000,), generator=g).float())
    x = torch.cat([x, torch.tensor([0.0, 1.0, -1.0, 2.0 ** -14, 2.0 ** -15, 3 * 2.0 ** -25, 2.0 ** -24])])
    want = x.to(BR.TORCH_DTYPE[fmt]).double()  # one rounding: x is an fp32 number
    assert torch.equal(BR.rnd(x.double(), fmt), want)
    # ties go to even: the midpoint of 1 and 1 + ulp, and of 1 + ulp and 1 + 2 ulp
    u = BR.ulp(torch.tensor([1.0]), fmt).item()
    assert BR.rnd(torch.tensor([1.0 + u / 2, 1.0 + 3 * u / 2]), fmt).tolist() == [1.0, 1.0 + 2 * u]


@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
def test_round_stage_bounds_every_value_of_the_interval(fmt):
    g = torch.Generator().manual_seed(1)
    n = 200000
    v = (torch.randn(n, generator=g) * 3).double()
    e = torch.rand(n, generator=g).double() * BR.ulp(v, fmt) * torch.tensor([1e-3, 0.3, 1.0, 3.0]).repeat(n // 4)
    vr, er = BR.round_stage(v, e, fmt)
    for t in (-1.0, -0.5, 0.0, 0.37, 1.0):
        assert bool(((BR.rnd(v + t * e, fmt) - vr).abs() <= er).all())
    assert 0.0 < BR.flip_share(er) < 1.0
    assert bool((er <= e + 2 * BR.ulp(v, fmt)).all())
    # no midpoint within e: the error is reset to zero
    far = ((v / BR.ulp(v, fmt)) % 1.0 - 0.5).abs() * BR.ulp(v, fmt) > 2 * e
    assert bool((er[far & (v.abs() > 1e-3)] == 0).all()) and int(far.sum()) > n // 10
    # across a binade boundary e + ulp(v) is NOT a bound; the stage's e_r is
    q = BR.ulp(torch.tensor([0.99]), fmt).item()
    v1, e1 = torch.tensor([1.0 - 0.51 * q]), torch.tensor([1.52 * q])
    vr1, er1 = BR.round_stage(v1, e1, fmt)
    x = v1 + 1.515 * q
    assert (BR.rnd(x, fmt) - vr1).item() == 3 * q > (e1 + q).item() and er1.item() == 3 * q


def test_assert_within_reports_and_returns_the_ratio():
    v = torch.arange(12.0, dtype=torch.float64).reshape(3, 4)
    e = torch.full_like(v, 0.5)
    assert BR.assert_within(v + 0.25, v, e, "ok") == 0.5
    assert BR.assert_within(v.clone(), v, None, "exact") == 0.0
    got = v.clone()
    got[1, 2] += 2.0
    got[2, 0] -= 1.0
    with pytest.raises(AssertionError) as ei:
        BR.assert_within(got, v, e, "two wrong")
    msg = str(ei.value)
    assert "2 of 12" in msg and "(1, 2)" in msg and "= 4" in msg
    got = v.clone()
    got[0, 0] = float("nan")
    with pytest.raises(AssertionError):
        BR.assert_within(got, v, e, "nan")
    # a broken reference cannot make the check vacuous
    for bad_v, bad_e in ((float("nan"), 0.5), (float("inf"), 0.5), (0.0, float("nan")), (0.0, float("inf")),
                         (0.0, -1.0)):
        v2, e2 = v.clone(), e.clone()
        v2[1, 1] += bad_v
        e2[1, 1] = bad_e
        with pytest.raises(AssertionError, match="reference v|bound e"):
            BR.assert_within(v.clone(), v2, e2, "broken reference")


# ---------------------------------------------------------------- soundness, every device shape
def _sound(emulate, ref, what):
    v, e = ref
    worst = [BR.assert_within(emulate(o), v, e, f"{what} [{o}]") for o in ORDERS]
    print(f"{what}: worst |emu - v| / e = {max(worst):.3f}, flips possible {BR.flip_share(e):.2e}")


@pytest.mark.parametrize("case", C.CONV_GEMM, ids=lambda c: "-".join(map(str, c[:8])))
def test_sound_conv_gemm(case):
    B, H, W, Cin, Cout, k, stride, dil, act, res, _, _ = case
    x, w, b, r = C.gen_conv(1, B, H, W, Cin, Cout, k, stride, dil, res)
    kw = dict(stride=stride, dil=dil, act=act, res=r)
    _sound(lambda o: C.conv_emulate(x, w, b, order=o, **kw), C.conv_bound(x, w, b, **kw), "conv_gemm")


@pytest.mark.parametrize("B,H,W,rate", C.TAP_GROUPED)
def test_sound_tap_grouped(B, H, W, rate):
    x, w, b, _ = C.gen_conv(5, B, H, W, 64, 96, 3, 1, rate)
    kw = dict(dil=rate, act="relu")
    _sound(lambda o: C.conv_emulate(x, w, b, order=o, **kw), C.conv_bound(x, w, b, **kw), "tap_grouped")


def _aspp_branches(seed, B, H, W, Cin, Cout):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, Cin, H, W, generator=g).to(torch.bfloat16)
    for k, rate in C.ASPP_BRANCHES:
        w = (torch.randn(Cout, Cin, k, k, generator=g) / (Cin * k * k) ** 0.5).to(torch.bfloat16)
        yield x, w, torch.randn(Cout, generator=g), rate


@pytest.mark.parametrize("shape", sorted({c[:5] for c in C.GROUPED_ASPP}) +
                         sorted({(B, 33, 33, 320, 256, "splitk") for B, _, _ in C.GROUPED_SPLITK}))
def test_sound_grouped_aspp(shape):
    """Split-K shares the bound: n is the full K, the partials are fp32."""
    for j, (x, w, b, rate) in enumerate(_aspp_branches(12 if len(shape) == 6 else 11, *shape[:5])):
        kw = dict(dil=rate, act="relu")
        _sound(lambda o: C.conv_emulate(x, w, b, order=o, **kw), C.conv_bound(x, w, b, **kw), f"aspp {j}")


@pytest.mark.parametrize("B,H,W,Cin,Cout,rate,grouped", C.TAP_CONV)
def test_sound_tap_conv(B, H, W, Cin, Cout, rate, grouped):
    x, w, b, _ = C.gen_conv(6, B, H, W, Cin, Cout, 3, 1, rate)
    kw = dict(dil=rate, act="relu")
    _sound(lambda o: C.conv_emulate(x, w, b, order=o, **kw), C.conv_bound(x, w, b, **kw), "tap_conv")


def test_sound_img_bias_and_bias_act():
    g = torch.Generator().manual_seed(2)
    x = torch.randn(3, 64, 5, 7, generator=g).to(torch.bfloat16)
    w = (torch.randn(48, 64, 1, 1, generator=g) / 8).to(torch.bfloat16)
    b, ib = torch.randn(48, generator=g), torch.randn(3, 48, generator=g)
    kw = dict(act="relu", img_bias=ib)
    _sound(lambda o: C.conv_emulate(x, w, b, order=o, **kw), C.conv_bound(x, w, b, **kw), "img_bias")
    g = torch.Generator().manual_seed(3)
    x = torch.randn(3 * 37, 264, generator=g).to(torch.bfloat16)
    b, ib = torch.randn(264, generator=g), torch.randn(3, 264, generator=g)
    for rows in (ib.repeat_interleave(37, 0), None):
        emu = x.float() + b
        emu = torch.relu(emu if rows is None else emu + rows).to(torch.bfloat16)
        v, e = C.bias_act_bound(x, b, rows, "relu")
        BR.assert_within(emu, v, e, "bias_act")


def _pw_inputs(M, Cin, Cout, res, img, n_out):
    g = torch.Generator().manual_seed(3)
    x = (torch.randn(M, Cin, generator=g) * 0.5).to(torch.bfloat16)
    w = (torch.randn(Cout, Cin, generator=g) / Cin ** 0.5).to(torch.bfloat16)
    b = torch.randn(Cout, generator=g)
    N = n_out or Cout
    r = torch.randn(M, N, generator=g).to(torch.bfloat16)[:, :Cout] if res else None
    ib = torch.randn(M // 121, N, generator=g).repeat_interleave(121, 0)[:, :Cout] if img else None
    return x, w, b, r, ib


@pytest.mark.parametrize("case", C.PW_CONV, ids=lambda c: "-".join(map(str, c[:3])))
def test_sound_pw_conv(case):
    M, Cin, Cout, act, res, img, _, _, n_out = case
    x, w, b, r, ib = _pw_inputs(M, Cin, Cout, res, img, n_out)
    kw = dict(act=act, res=r, img_rows=ib)
    _sound(lambda o: C.mat_emulate(x, w, b, order=o, **kw), C.mat_bound(x, w, b, **kw), "pw_conv")


def test_sound_pw_conv_fp16_out():
    M, Cin, Cout = C.PW_FP16
    g = torch.Generator().manual_seed(12)
    x = (torch.randn(M, Cin, generator=g) * 0.5).to(torch.bfloat16)
    w = (torch.randn(Cout, Cin, generator=g) / Cin ** 0.5).to(torch.bfloat16)
    b = torch.randn(Cout, generator=g)
    kw = dict(act="relu6", fmt="fp16")
    _sound(lambda o: C.mat_emulate(x, w, b, order=o, **kw), C.mat_bound(x, w, b, **kw), "pw_conv fp16")


def _dw_inputs(seed, B, C_, H, W, relu6_in=False):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, C_, H, W, generator=g)
    x = (F.relu6(x * 2) if relu6_in else x).to(torch.bfloat16)
    return g, x, torch.randn(C_, 1, 3, 3, generator=g) / 3


@pytest.mark.parametrize("B,H,W,C_,stride,dil", C.DEPTHWISE)
def test_sound_depthwise(B, H, W, C_, stride, dil):
    g, x, w = _dw_inputs(3, B, C_, H, W)
    b = torch.randn(C_, generator=g)
    kw = dict(stride=stride, dil=dil, act="relu6", groups=C_)
    _sound(lambda o: C.conv_emulate(x, w, b, order=o, **kw), C.conv_bound(x, w, b, **kw), "depthwise")


def _dw_project_case(hid, cout, stride, dil, res):
    g, x, wd = _dw_inputs(10, 2, hid, 21, 21, relu6_in=True)
    bd = torch.randn(hid, generator=g) * 0.1
    wp = (torch.randn(cout, hid, generator=g) / hid ** 0.5).to(torch.bfloat16)
    bp = torch.randn(cout, generator=g) * 0.1
    OH = (21 - 1) // stride + 1
    r = torch.randn(2, cout, OH, OH, generator=g).to(torch.bfloat16) if res else None
    return x, wd, bd, wp, bp, r


def _dw_project_emulate(x, wd, bd, wp, bp, r, stride, dil, order, hidden_hook=None):
    d = C.conv_emulate(x, wd, bd, stride=stride, dil=dil, act="relu6", groups=x.shape[1], order=order)
    if hidden_hook is not None:
        d = hidden_hook(d)
    return C.conv_emulate(d, wp[:, :, None, None], bp, res=r, order=order)


@pytest.mark.parametrize("hid,cout,stride,dil,res", C.DW_PROJECT)
def test_sound_dw_project(hid, cout, stride, dil, res):
    x, wd, bd, wp, bp, r = _dw_project_case(hid, cout, stride, dil, res)
    hidp, outp = C.dw_project_bound(x, wd, bd, wp, bp, stride=stride, dil=dil, res=r)
    _sound(lambda o: _dw_project_emulate(x, wd, bd, wp, bp, r, stride, dil, o), outp, "dw_project")
    # the resets keep the bound tight: a flip is possible where a midpoint lies within e, a share
    # of about 2 e / ulp = 4 * 13 * 2^-24 / 2^-8 * (sum |x w| / |sum x w|), a few 1e-3
    assert BR.flip_share(hidp[1]) < 1e-2


def _fused_sound(x, P, tile, what):
    v, e = C.fused_ir_bound(x, P, tile=tile)
    worst = [BR.assert_within(C.fused_ir_emulate(x, P, tile=tile, order=o), v, e, what) for o in ORDERS]
    print(f"{what}: worst |emu - v| / e = {max(worst):.3f}, flips possible {BR.flip_share(e):.2e}")
    return v, e


@pytest.mark.parametrize("cin,cout,t,stride,H", C.FUSED_IR)
def test_sound_fused_ir(cin, cout, t, stride, H):
    _, P = C.ir_block(cin, cout, t, stride, 1, cin + cout, "cpu")
    x = torch.randn(2, cin, H, H + 6, generator=torch.Generator().manual_seed(9)).to(torch.bfloat16)
    _fused_sound(x, P, False, "fused_ir row kernel")


@pytest.mark.parametrize("cin,cout,stride,dil,H,tile", C.FUSED_IR_TILE, ids=lambda v: str(v).replace(" ", ""))
def test_sound_fused_ir_tile(cin, cout, stride, dil, H, tile):
    _, P = C.ir_block(cin, cout, 1 if cout == 16 else 6, stride, dil, cin + 3 * cout + dil, "cpu")
    x = torch.randn(2, cin, H, H + 4, generator=torch.Generator().manual_seed(19)).to(torch.bfloat16)
    _fused_sound(x, P, True, "fused_ir tile kernel")


@pytest.mark.parametrize("cin,cout,dil,H", sorted({(c[0], c[1], c[2], c[3]) for c in C.FUSED_IR_STREAM} |
                                                  {(160, c[0], 2, c[1]) for c in C.FUSED_IR_LATTICE}))
def test_sound_fused_ir_stream(cin, cout, dil, H):
    """The stream kernel's shapes (raster and lattice spans compute the same chain per pixel;
    the span count only cuts the map), from its own packed chunk images."""
    from test_fused_span_cpu import _block, pack_block
    torch.manual_seed(cin + cout + H)  # _block draws the BN statistics from the global generator
    blk, spec = _block(cin, cout, dil, seed=cin * 5 + cout + dil)
    P = dict(C.unpack_fused_span(pack_block(blk, spec)), dil=dil, residual=spec.residual)
    x = torch.randn(3, cin, H, 33, generator=torch.Generator().manual_seed(23)).to(torch.bfloat16)
    v, _ = _fused_sound(x, P, True, "fused_ir_stream")
    with torch.no_grad():  # the unpacked operands are the block's: the reference is near the fp32 block
        ref = blk(x.float())
    assert ((v.float() - ref).norm() / ref.norm()).item() < 1e-2


@pytest.mark.parametrize("cin,cout,stride,H,W", C.FUSED_IR_BAND)
def test_sound_fused_ir_band(cin, cout, stride, H, W):
    """Band and slice kernels: the emulation accumulates from zero and adds the bias last, as
    they do, and so does the flip-aware reference. The bound without resets (the minimum for
    these kernels, whatever their order) must contain the flip-aware interval everywhere and
    admit the bias-first order too; it stays below half the output's spread."""
    from test_fused_band_cpu import band_block, pack_band
    torch.manual_seed(cin + cout + H)  # band_block draws the BN statistics from the global generator
    blk, spec = band_block(cin, cout, stride, seed=cin * 5 + cout + stride)
    P = C.unpack_fused_band(pack_band(blk, spec), stride, spec.residual)
    x = torch.randn(2, cin, H, W, generator=torch.Generator().manual_seed(31)).to(torch.bfloat16)
    v, e = _fused_sound(x, P, True, "fused_ir_band")
    vl, el = C.fused_ir_bound(x, dict(P, chain="loose"), tile=True)
    assert bool(((v - vl).abs() + e <= el).all())
    BR.assert_within(C.fused_ir_emulate(x, dict(P, chain="exact"), tile=True), vl, el, "bias-first order")
    with torch.no_grad():
        ref = blk(x.float())
    assert ((v.float() - ref).norm() / ref.norm()).item() < 1e-2
    print(f"fused_ir_band: flip-aware max e {float(e.max()):.4f}; without resets max e {float(el.max()):.3f}, "
          f"output std {float(v.std()):.3f}")
    assert float(el.max()) < 0.5 * float(v.std()), (float(el.max()), float(v.std()))


@pytest.mark.parametrize("cam,k,cout", C.STEM)
def test_sound_stem(cam, k, cout):
    """stem_conv (fp32 pixels and weights) and stem_mfma (both rounded to bf16), per-tap
    partial convs as the second order."""
    frames, lx, ly, w, b = C.gen_stem(cam, k, cout)
    for bf16 in (False, True):
        x = C.stem_pixels(frames, lx, ly, bf16)
        wk = w.to(torch.bfloat16) if bf16 else w
        _sound(lambda o: C.conv_emulate(x, wk, b, stride=2, act="relu6", order=o),
               C.stem_bound(x, w, b, act="relu6", bf16_weights=bf16), "stem_mfma" if bf16 else "stem_conv")


@pytest.mark.parametrize("cam,H,seed", C.STEM_BLOCK0_INPUTS)
def test_sound_stem_block0(cam, H, seed):
    """Every input of test_stem_block0_fused and every bounded one of test_stem_band, from
    ``pack_stem_block0``'s own operands; the reference stays near the fp32 torch layers."""
    from semantic_segmentation_server_amd.ops import reference_ops as R
    stem, blk, frames, lx, ly, P = C.stem_block0_case(cam, H, seed, "cpu")
    x = C.stem_pixels(frames, lx, ly, True)
    v, e = C.stem_block0_bound(x, P)
    _sound(lambda o: C.stem_block0_emulate(x, P, o), (v, e), "stem_block0")
    import numpy as np
    with torch.no_grad():
        ref = blk(stem(R.preprocess(frames, torch.from_numpy(np.array(lx)), torch.from_numpy(np.array(ly)))))
    assert ((v.float() - ref).norm() / ref.norm()).item() < 1e-2


def test_teeth_stem_block0_hidden_value_dropped():
    """One fp16 depthwise value of stem + block 0 lost before the 32-term projection. The site
    is the first hidden element in raster order with d >= 0.5 that reaches, through a projection
    weight of at least 0.25, an output where no flip is possible: that output moves by at least
    0.125, eight bf16 ulps of a value below 4."""
    cam, H, seed = C.STEM_BLOCK0_INPUTS[0]
    _, _, frames, lx, ly, P = C.stem_block0_case(cam, H, seed, "cpu")
    x = C.stem_pixels(frames, lx, ly, True)
    v, e = C.stem_block0_bound(x, P)
    ws = P["ws"].float().reshape(32, 12, 4)[:, :9, :3].reshape(32, 3, 3, 3).permute(0, 3, 1, 2)
    h = C.conv_emulate(x, ws, P["bs"], stride=2, act="unit", fmt="fp16")
    blk = dict(Cin=32, Cout=16, hidP=32, stride=1, act="unit", we=None, residual=False,
               wd_h=P["wd_h"], bd_h=P["bd_h"], wp_h=P["wp_h"], bp=P["bp"])

    def hook(d):
        sure = ((e == 0) & (v.abs() < 4)).double().permute(0, 2, 3, 1)
        reach = (sure @ (P["wp_h"].double().abs() >= 0.25).double()).permute(0, 3, 1, 2) > 0
        d = d.clone()
        d[_first((d >= 0.5) & reach)] = 0.0
        return d

    BR.assert_within(C.fused_ir_emulate(h, blk, tile=True), v, e, "unmutated")
    _rejected(C.fused_ir_emulate(h, blk, tile=True, hidden_hook=hook), v, e, "hidden value dropped", 16)


@pytest.mark.parametrize("tile", [False, True])
def test_teeth_fused_hidden_element_dropped(tile):
    """160 -> 960 -> 160 (the row kernel's bf16 chain, and the tile kernel's fp16 internals at
    dilation 2). Two roundings upstream of a 960-term projection, each behind the worst-case
    fp32 bound of its own sum, leave a flip possible at most outputs: e is about one output ulp
    there, too wide for a 4 ulp hidden error (tests of ``dw_project`` catch that one, one
    rounding upstream) but far below one lost depthwise value, which the norm cannot see."""
    _, P = C.ir_block(160, 160, 6, 1, 2 if tile else 1, 7, "cpu")
    x = torch.randn(2, 160, 17, 19, generator=torch.Generator().manual_seed(19)).to(torch.bfloat16)
    v, e = _fused_sound(x, P, tile, "unmutated")

    def hook(d):
        d = d.clone()
        d[_first(d >= 3)] = 0.0
        return d

    got = C.fused_ir_emulate(x, P, tile=tile, hidden_hook=hook)
    _rejected(got, v, e, "hidden value dropped", 160)
    ref = C.fused_ir_emulate(x, P, tile=tile).float()
    assert ((got.float() - ref).norm() / ref.norm()).item() < 1e-2  # invisible to the 2e-2 norm bound


@pytest.mark.parametrize("hid,cout,stride,dil,res", C.DW_PROJ_FUSED)
def test_sound_dw_proj_fused(hid, cout, stride, dil, res):
    g = torch.Generator().manual_seed(11)
    x = F.relu6(torch.randn(3, hid, 19, 19, generator=g) * 2).to(torch.bfloat16)
    wd = torch.randn(hid, 1, 3, 3, generator=g) / 3
    bd = torch.randn(hid, generator=g) * 0.1
    wp = (torch.randn(cout, hid, generator=g) / hid ** 0.5).to(torch.bfloat16)
    bp = torch.randn(cout, generator=g) * 0.1
    OH = (19 - 1) // stride + 1
    r = torch.randn(3, cout, OH, OH, generator=g).to(torch.bfloat16) if res else None
    v, e = C.dw_proj_fused_bound(x, wd, bd, wp, bp, stride=stride, dil=dil, res=r)
    # the fused tile emulation with no expansion is this kernel: fp16 input, chain, fp16 MFMA
    P = dict(Cin=hid, Cout=cout, stride=stride, dil=dil, hidP=hid, we=None, residual=False,
             wd_h=wd.reshape(hid, 9).t().half(), bd_h=bd.half(), wp_h=wp.half(), bp=bp)
    for o in ORDERS:
        BR.assert_within(C.fused_ir_emulate(x, P, tile=True, order=o, res=r), v, e, f"dw_proj_fused [{o}]")
    print(f"dw_proj_fused: flips possible {BR.flip_share(e):.2e}")


@pytest.mark.parametrize("M,HW,ncls,ldo,img", C.ASPP_HEAD[1:])
def test_sound_aspp_head(M, HW, ncls, ldo, img):
    """The B = 32 head (34848 rows) is the same arithmetic per row as these; its device test
    shares their reference function."""
    cat, wp, bp, wl, bl, ib = C.gen_aspp_head(M, HW, ncls, img)
    rows = None if ib is None else ib.repeat_interleave(HW, 0)
    v, e = C.aspp_head_bound(cat, wp, bp, wl, bl, rows)
    for o in ORDERS:
        proj = C.mat_emulate(cat, wp, bp, act="relu", img_rows=rows, order=o)
        BR.assert_within(C.mat_emulate(proj, wl, bl, order=o), v, e, f"aspp_head [{o}]")
    print(f"aspp_head: flips possible {BR.flip_share(e):.2e}")


@pytest.mark.parametrize("B,N,K,bias", C.MATVEC)
def test_sound_matvec(B, N, K, bias):
    g = torch.Generator().manual_seed(N)
    x, w = torch.randn(B, K, generator=g), torch.randn(N, K, generator=g)
    b = torch.randn(N, generator=g) if bias else None
    kw = dict(act="relu", fmt=None)
    _sound(lambda o: C.mat_emulate(x, w, b, order=o, **kw), C.mat_bound(x, w, b, **kw), "matvec")


@pytest.mark.parametrize("B,h,w,C_,N", C.ASPP_POOL)
def test_sound_aspp_pool(B, h, w, C_, N):
    g = torch.Generator().manual_seed(11)
    x = (torch.randn(B, C_, h, w, generator=g) + 0.3).to(torch.bfloat16)
    w1, b1 = torch.randn(N, C_, generator=g) / C_ ** 0.5, torch.randn(N, generator=g)
    w2 = torch.randn(N, N, generator=g) / N ** 0.5
    v, e = C.aspp_pool_bound(x, w1, b1, w2)
    xf = x.float()
    for gap in (xf.mean((2, 3)), xf.reshape(B, C_, -1).cumsum(2)[..., -1] * (1.0 / (h * w))):
        BR.assert_within(F.relu(gap @ w1.t() + b1) @ w2.t(), v, e, "aspp_pool")


def test_dw_chain_fp16_past_two_to_the_fifth():
    """Below 2^5 the chain is exact in float64 and an exact input stays exact (e None, as
    before); once a partial sum reaches 2^5 (BN-folded depthwise weights of the plan tests) the
    chain carries float64's own 2^-53 relative rounding, and still contains the emulation."""
    g = torch.Generator().manual_seed(3)
    x = (torch.rand(2, 4, 9, 9, generator=g) * 6).half()
    wd = (torch.rand(4, 9, generator=g) * 0.5 + 0.75).half()   # 9 taps of ~1 on values up to 6: sums to ~50
    bd = torch.randn(4, generator=g).half()
    for scale, big in ((1.0, True), (0.25, False)):
        w = (wd.float() * scale).half()
        for last in (False, True):
            v, e = C.dw_chain_fp16((x.double(), None), w, bd, stride=1, dil=1, act=None, bias_last=last)
            assert (float(v.abs().max()) >= 32.0) == big
            assert (e is not None) == big
            P = dict(Cin=4, Cout=4, stride=1, dil=1, hidP=4, we=None, residual=False, wd_h=w.t(), bd_h=bd,
                     wp_h=torch.eye(4).half(), bp=torch.zeros(4), act="relu6", chain="bias_last" if last else None)
            d = []
            C.fused_ir_emulate(x, P, tile=True, hidden_hook=lambda t: d.append(t) or t)
            vc, ec = BR.act((v, e), "relu6")
            BR.assert_within(d[0], vc, ec, f"chain scale {scale} bias_last {last}")


@pytest.mark.parametrize("B,H,W,C_", C.MAXPOOL)
def test_sound_maxpool(B, H, W, C_):
    """The max pool is exact: a correct kernel, written as the explicit maximum over the nine
    shifted views of the -inf-padded map, equals the reference bit for bit (all-negative maps
    included: the padding never wins); a window that misses one tap is rejected."""
    g = torch.Generator().manual_seed(H * W)
    x = (torch.randn(B, C_, H, W, generator=g) - 1.0).to(torch.bfloat16)
    v, e = C.maxpool_bound(x)
    assert e is None
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    assert v.shape == (B, C_, OH, OW)
    xp = F.pad(x.float(), (1, 1, 1, 1), value=float("-inf"))
    taps = [xp[:, :, i:i + 2 * OH - 1:2, j:j + 2 * OW - 1:2] for i in range(3) for j in range(3)]
    BR.assert_within(torch.stack(taps).amax(0).to(torch.bfloat16), v, e, "maxpool")
    short = torch.stack(taps[:-1]).amax(0)
    if bool((short.double() != v).any()):
        assert bool(BR.violations(short, v, e).any())
    else:
        assert H == 1  # a single row: the third row of taps is padding


def test_sound_gap_and_its_matvec():
    """test_maxpool_gap_matvec: the fp32 mean of 31 x 29 bf16 values in two orders (pairwise
    and a running sum), and the fp32 matvec of that GAP."""
    g = torch.Generator().manual_seed(6)
    x = torch.randn(2, 64, 31, 29, generator=g).to(torch.bfloat16)
    wm, bm = torch.randn(40, 64, generator=g), torch.randn(40, generator=g)
    gv, ge = C.gap_bound(x)
    xf = x.float()
    for gap in (xf.mean((2, 3)), xf.reshape(2, 64, -1).cumsum(2)[..., -1] * (1.0 / (31 * 29))):
        BR.assert_within(gap, gv, ge, "global_avgpool")
        for o in ORDERS:
            BR.assert_within(C.mat_emulate(gap, wm, bm, act="relu", fmt=None, order=o),
                             *C.mat_bound(gv, wm, bm, act="relu", fmt=None, x_err=ge), "matvec of the GAP")
    got = xf.mean((2, 3))
    # one pixel left out of one channel's mean: the largest, over 2 of 899 values of spread 1
    got[1, 7] = (xf[1, 7].sum() - xf[1, 7].flatten()[xf[1, 7].abs().argmax()]) / (31 * 29)
    _rejected(got, gv, ge, "pixel dropped", 1)


# ---------------------------------------------------------------- teeth
def _first(mask):
    assert bool(mask.any()), "no site at which the mutation changes a value where e = 0"
    return tuple(int(i) for i in torch.nonzero(mask)[0])


def _rejected(got, v, e, what, at_most):
    with pytest.raises(AssertionError) as ei:
        BR.assert_within(got, v, e, what)
    n = int(BR.violations(got, v, e).sum())
    assert 1 <= n <= at_most and f"{n} of {v.numel()}" in str(ei.value)


TEETH = [C.CONV_GEMM[5], C.CONV_GEMM[8], C.CONV_GEMM[10]]  # dil 6 on 33 x 33; stride 2; tiny, dil 2


@pytest.mark.parametrize("case", TEETH, ids=lambda c: "-".join(map(str, c[:8])))
def test_teeth_single_mutations(case):
    B, H, W, Cin, Cout, k, stride, dil, act, res, _, _ = case
    x, w, b, r = C.gen_conv(1, B, H, W, Cin, Cout, k, stride, dil, res)
    kw = dict(stride=stride, dil=dil, act=act, res=r)
    v, e = C.conv_bound(x, w, b, **kw)
    emu = C.conv_emulate(x, w, b, **kw)
    BR.assert_within(emu, v, e, "unmutated")
    exact = e == 0
    OH, OW = emu.shape[-2:]
    # (1) one corner output pixel computed with its centre tap dropped
    short = F.relu(C.sum_taps(x.float(), w.float(), stride, dil, skip=(1, 1)) + b[None, :, None, None]) \
        .to(torch.bfloat16)
    corners = torch.zeros_like(exact)
    corners[:, :, 0::OH - 1, 0::OW - 1] = True
    bb, _, yy, xx = _first(corners & exact & (short != emu))
    got = emu.clone()
    got[bb, :, yy, xx] = short[bb, :, yy, xx]
    _rejected(got, v, e, "dropped tap", Cout)
    # (2) one element replaced by its right-hand neighbour's value
    right = torch.roll(emu, -1, 3)
    m = exact & (right != emu)
    m[..., -1] = False
    i = _first(m)
    got = emu.clone()
    got[i] = right[i]
    _rejected(got, v, e, "right neighbour", 1)
    # (3) two adjacent output channels swapped at one pixel
    nxt = torch.roll(emu, -1, 1)
    m = exact & (nxt != emu)
    m[:, -1] = False
    bb, cc, yy, xx = _first(m)
    got = emu.clone()
    got[bb, cc, yy, xx], got[bb, cc + 1, yy, xx] = emu[bb, cc + 1, yy, xx], emu[bb, cc, yy, xx]
    _rejected(got, v, e, "channel swap", 2)


@pytest.mark.parametrize("B,H,W,rate", C.TAP_GROUPED[:1] + C.TAP_GROUPED[3:])
def test_teeth_padding_row_written(B, H, W, rate):
    """The tap-grouped GEMM walks rows of ``perm``; a row of -1 is padding and writes nothing.
    A kernel that writes it anyway stores act(bias) (every tap masked) at the pixel the index
    -1 lands on, the last one of the buffer."""
    from semantic_segmentation_server_amd.ops.hip_ops import tap_group_perm
    x, w, b, _ = C.gen_conv(5, B, H, W, 64, 96, 3, 1, rate)
    v, e = C.conv_bound(x, w, b, dil=rate, act="relu")
    emu = C.conv_emulate(x, w, b, dil=rate, act="relu")
    perm = tap_group_perm(B, H, W, 3, rate, 128)
    assert int((perm == -1).sum()) > 0
    rows = emu.permute(0, 2, 3, 1).reshape(B * H * W, 96).clone()
    stray = F.relu(b).to(torch.bfloat16)
    assert bool(((stray != rows[-1]) & (e.permute(0, 2, 3, 1).reshape(-1, 96)[-1] == 0)).any())
    rows[int(perm[perm == -1][0])] = stray
    _rejected(rows.reshape(B, H, W, 96).permute(0, 3, 1, 2), v, e, "padding row", 96)


@pytest.mark.parametrize("hid,cout,stride,dil,res", [C.DW_PROJECT[0], C.DW_PROJECT[4]])
def test_teeth_hidden_element_four_ulp(hid, cout, stride, dil, res):
    """One bf16 depthwise value 4 ulp off before the projection: the first hidden element
    in raster order with 2 <= d < 6 (4 ulp = 2^-4 or 2^-5, times a projection weight)."""
    x, wd, bd, wp, bp, r = _dw_project_case(hid, cout, stride, dil, res)
    _, (v, e) = C.dw_project_bound(x, wd, bd, wp, bp, stride=stride, dil=dil, res=r)

    def hook(d):
        i = _first((d >= 2) & (d < 6))
        d = d.clone()
        d[i] = (d[i].double() + 4 * BR.ulp(d[i].double(), "bf16")).to(torch.bfloat16)
        return d

    BR.assert_within(_dw_project_emulate(x, wd, bd, wp, bp, r, stride, dil, "whole"), v, e, "unmutated")
    _rejected(_dw_project_emulate(x, wd, bd, wp, bp, r, stride, dil, "whole", hook), v, e, "hidden + 4 ulp", cout)
