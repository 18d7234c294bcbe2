"""The ASPP image-pooling branch as work items of the grouped branch GEMM (conv_gemm_grouped's
``pool``): for every variant that offers the fused form, img_bias equals the separate kernels'
(K.aspp_pool) bit for bit and the concat buffer equals the same variant's unfused launch bit
for bit -- on a first launch and on a second one into poisoned outputs.

The kernels are specialised to the ASPP of the models: C = 320, A = 256, rates 6 / 12 / 18.
(1, 5, 7) has slices of one pixel and of two (HW = 35); (1, 5, 5) has HW < 32, so some slices
are empty and HW * sl / 32 repeats; (1, 9, 9) and (3, 9, 9) run more than one pool item and
the image offset; (2, 33, 33) is the headline feature map (34- and 35-pixel slices: full
batches of the chain walk plus a tail)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
C, A = 320, 256
SHAPES = [(1, 9, 9), (3, 9, 9), (2, 33, 33), (1, 5, 7), (1, 5, 5)]


def _hip():
    from semantic_segmentation_server_amd.ops import hip_ops
    return hip_ops


_CASES = {}


def _case(B, h, w):
    """Inputs, weights and the separate kernels' img_bias (computed once per shape)."""
    if (B, h, w) in _CASES:
        return _CASES[(B, h, w)]
    K = _hip()
    g = torch.Generator().manual_seed(100 * B + 10 * h + w)
    x = (torch.randn(B, h, w, C, generator=g) + 0.3).to(torch.bfloat16).to(DEV)
    ws = []
    for k in (1, 3, 3, 3):
        wk = (torch.randn(A, k, k, C, generator=g) / (C * k * k) ** 0.5).to(torch.bfloat16).to(DEV)
        ws.append((wk, torch.randn(A, generator=g).to(DEV), k))
    w1t = (torch.randn(C, A, generator=g) / C ** 0.5).to(DEV)
    b1 = torch.randn(A, generator=g).to(DEV)
    w2t = (torch.randn(A, A, generator=g) / A ** 0.5).to(DEV)
    ref = torch.full((B, A), float("nan"), device=DEV)
    K.aspp_pool(x, K.gap_workspace(B, C, DEV), w1t, b1, w2t, ref, B=B, HW=h * w, C=C, N=A)
    torch.cuda.synchronize()
    assert torch.isfinite(ref).all()
    _CASES[(B, h, w)] = dict(x=x, ws=ws, w1t=w1t, b1=b1, w2t=w2t, ref=ref)
    return _CASES[(B, h, w)]


def _convs(K, cs, B, h, w, variant, out):
    BM = K.GROUP_TILE[variant][0]
    return [dict(x=cs["x"], w=wk, bias=bk, out=out, B=B, IH=h, IW=w, Cin=C, OH=h, OW=w, Cout=A, k=k,
                 dil=rate, ldo=4 * A, co_off=j * A, act="relu",
                 perm=K.tap_group_perm(B, h, w, 3, rate, BM, DEV) if k == 3 else None)
            for j, ((wk, bk, k), rate) in enumerate(zip(cs["ws"], (1, 6, 12, 18)))]


def _bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def _run_both(B, h, w, variant, ks=1, inl=False):
    K = _hip()
    cs = _case(B, h, w)
    cat_u = torch.full((B, h, w, 4 * A), float("nan"), dtype=torch.bfloat16, device=DEV)
    cat_f = torch.full_like(cat_u, float("nan"))
    ib = torch.full((B, A), float("nan"), device=DEV)
    cu, cf = _convs(K, cs, B, h, w, variant, cat_u), _convs(K, cs, B, h, w, variant, cat_f)
    order = K.grouped_tile_order(cu, variant, DEV, ks=ks)
    order_p = K.grouped_tile_order(cf, variant, DEV, ks=ks, pool=B)
    assert order_p.numel() == order.numel() + B
    kw = {}
    if ks > 1:
        kw = dict(ks=ks, part=torch.full((ks * B * h * w * 4 * A,), float("nan"), device=DEV),
                  bias_cat=torch.cat([b for _, b, _ in cs["ws"]]),
                  cnt=torch.zeros(4 * 64, dtype=torch.int32, device=DEV) if inl else None)
    item = dict(x=cs["x"], w1t=cs["w1t"], b1=cs["b1"], w2t=cs["w2t"], img_bias=ib, B=B, HW=h * w, C=C, N=A)
    K.conv_gemm_grouped(cu, order, variant, **kw)
    torch.cuda.synchronize()
    assert not torch.isnan(cat_u.float()).any()
    for launch in range(2):  # the second launch writes into poisoned outputs
        cat_f.fill_(float("nan"))
        ib.fill_(float("nan"))
        K.conv_gemm_grouped(cf, order_p, variant, pool=item, **kw)
        torch.cuda.synchronize()
        assert torch.equal(_bits(ib), _bits(cs["ref"])), (variant, launch)
        assert torch.equal(_bits(cat_f), _bits(cat_u)), (variant, launch)
        if kw.get("cnt") is not None:
            assert int(kw["cnt"].abs().sum()) == 0


@pytest.mark.parametrize("B,h,w", SHAPES)
def test_fused_pool_bit_identical(B, h, w):
    K = _hip()
    assert K.GROUP_POOL_VARIANTS, "no grouped variant offers the fused form"
    for variant in K.GROUP_POOL_VARIANTS:
        _run_both(B, h, w, variant)


@pytest.mark.parametrize("variant,ks,inl", [(5, 6, False), (5, 6, True), (17, 2, True)])
def test_fused_pool_splitk_batch1(variant, ks, inl):
    """Split-K launches (the batch-1 picks): pool items carry K slice 0, touch no partial and
    draw no ticket."""
    assert variant in _hip().GROUP_POOL_VARIANTS
    _run_both(1, 9, 9, variant, ks=ks, inl=inl)
    _run_both(1, 33, 33, variant, ks=ks, inl=inl)


def test_pool_items_are_checked():
    """Pool operands without pool entries (and the reverse), and a variant that carries no
    pool items, are refused before any launch."""
    K = _hip()
    cs = _case(1, 9, 9)
    cat = torch.zeros((1, 9, 9, 4 * A), dtype=torch.bfloat16, device=DEV)
    ib = torch.zeros((1, A), device=DEV)
    item = dict(x=cs["x"], w1t=cs["w1t"], b1=cs["b1"], w2t=cs["w2t"], img_bias=ib, B=1, HW=81, C=C, N=A)
    v = K.GROUP_POOL_VARIANTS[0]
    convs = _convs(K, cs, 1, 9, 9, v, cat)
    with pytest.raises(ValueError, match="pool item"):
        K.conv_gemm_grouped(convs, K.grouped_tile_order(convs, v, DEV), v, pool=item)
    with pytest.raises(ValueError, match="pool item"):
        K.conv_gemm_grouped(convs, K.grouped_tile_order(convs, v, DEV, pool=1), v)
    convs11 = _convs(K, cs, 1, 9, 9, 11, cat)
    with pytest.raises(ValueError, match="pool items need"):
        K.conv_gemm_grouped(convs11, K.grouped_tile_order(convs11, 11, DEV, pool=1), 11, pool=item)


def test_fused_plan_copies_on_two_streams():
    """Two copies of a plan whose aspp.branches pick is a fused form, on two streams at once
    (pool items of one copy share CUs with the other copy's kernels): the label maps equal the
    sequential runs of the separate-pooling pick, frame for frame."""
    import numpy as np
    from semantic_segmentation_server_amd import config as Cfg
    from semantic_segmentation_server_amd.models.plan import Choice
    from semantic_segmentation_server_amd.runtime.engine import Engine
    from semantic_segmentation_server_amd.runtime.sources import SyntheticSource
    eng = Engine(Cfg.Config(input_size=257, batch=2, backend="hip", graph=True, min_area_ratio=0.002),
                 torch.device(DEV))
    src = SyntheticSource(160, 120, seed=7, pool=4)
    eng.set_camera(160, 120)
    hm = eng._hip_model
    fr = [torch.from_numpy(np.ascontiguousarray(src.read_batch(2)[0])).to(DEV) for _ in range(3)]
    hm.segment(fr[0], eng.lut_x, eng.lut_y)
    plans = [hm._plan(2, 120, 160, part)[0] for part in range(2)]
    br = [next(op for op in ops if isinstance(op, Choice) and op.name == "aspp.branches") for ops in plans]
    names = [n for n, _ in br[0].variants]
    fused = [n for n in names if n.endswith("+pool")]
    assert fused and "grouped_v15+pool" in fused, names
    for c in br:
        c.pick = names.index("grouped_v15")
    ref = [hm.segment(f, eng.lut_x, eng.lut_y, part=0).clone() for f in fr]
    for c in br:
        c.pick = names.index("grouped_v15+pool")
    for part in range(2):  # first launches outside the loop
        hm.segment(fr[0], eng.lut_x, eng.lut_y, part=part)
    torch.cuda.synchronize()
    ss = [torch.cuda.Stream() for _ in range(2)]
    labs = [torch.empty_like(ref[0]) for _ in range(2)]
    bad = torch.zeros((), dtype=torch.int64, device=DEV)
    for rep in range(30):
        for part in range(2):
            with torch.cuda.stream(ss[part]):
                hm.segment(fr[(rep + part) % 3], eng.lut_x, eng.lut_y, out=labs[part], part=part)
        torch.cuda.synchronize()
        for part in range(2):
            bad += (labs[part] != ref[(rep + part) % 3]).any()
    assert int(bad) == 0, f"{int(bad)} of 60 concurrent fused runs differ from the separate-pooling label maps"
