"""DeepLabv3 forward on the hand-written gfx950 kernels.

The torch model (``models/deeplab.py``) is the weight source and the numerics
reference; this module folds BatchNorm into every conv, packs the weights into
the kernels' layouts once, and executes the network as a fixed list of kernel
launches over static NHWC bf16 buffers (allocated per (batch, camera) on first
use, outside any graph capture; ``models/plan.py``). The engine captures the whole
list into one hipGraph.

Layout decisions (MI355X-first, not a translation of the tflite graph):
  * NHWC bf16 activations, fp32 accumulation; 1x1/3x3 dense convs are MFMA
    implicit GEMMs (``conv_gemm``) with bias/activation/residual fused in the
    epilogue; depthwise convs are vectorised VALU kernels (8 channels per lane).
  * Letterbox preprocessing is fused into the stem conv: the uint8 camera frame
    is read through the resize LUTs, so the 513x513x3 model input never exists.
  * ASPP is concat-free: each branch writes its channel slice of one buffer; the
    image-pooling branch (spatially constant) is folded through its slice of the
    projection weights into a per-image bias of the projection GEMM.
  * Logits are written with a padded channel stride (ld 24 for 21 classes) and
    upsampled + argmax'ed in one kernel.

Plan building: one method per network stage (returns its ops and the running ``(x, h, w,
c)``); per MobileNetV2 block one generator per kernel family (returns ``(variant, [ops])``).
"""
from __future__ import annotations

import os
from types import SimpleNamespace
from typing import Callable, Dict, List, Optional, Tuple

import torch

from ..ops import fused_band as FB
from ..ops import fused_span as FS
from ..ops import hip_ops as K
from ..ops import row_repeat as RR
from ..ops.hip_ops import conv_out_hw
from .deeplab import DeepLabV3
from .layers import ConvBNAct
from .mobilenetv2 import MobileNetV2Backbone
from .plan import TUNE_FILE_DEFAULT, Choice, HipPlanModel  # noqa: F401 (the tune file: tests, tools)


def _pack_dense(layer: ConvBNAct, dev) -> Tuple[torch.Tensor, torch.Tensor]:
    w, b = layer.fold()
    # [Cout, Cin, kh, kw] -> [Cout, kh, kw, Cin]
    return (w.permute(0, 2, 3, 1).contiguous().to(dev, torch.bfloat16),
            b.contiguous().to(dev, torch.float32))


def _pack_dw(layer: ConvBNAct, dev) -> Tuple[torch.Tensor, torch.Tensor]:
    w, b = layer.fold()  # [C, 1, 3, 3]
    return (w.reshape(w.shape[0], 9).t().contiguous().to(dev, torch.float32),
            b.contiguous().to(dev, torch.float32))


def _pack_stem(layer: ConvBNAct, dev) -> Tuple[torch.Tensor, torch.Tensor]:
    w, b = layer.fold()  # [Cout, 3, k, k] -> [k, k, 3, Cout]
    return (w.permute(2, 3, 1, 0).reshape(-1, w.shape[0]).contiguous().to(dev, torch.float32),
            b.contiguous().to(dev, torch.float32))


def _fold_block(m) -> tuple:
    """The folded layers of an inverted-residual block as the fused kernels' packers take
    them: (we, be, wd, bd, wp, bp); we = be = None for a block without expansion."""
    ew = eb = None
    if m.expand is not None:
        ew, eb = m.expand.fold()
        ew = ew[:, :, 0, 0]
    dwf, dbf = m.dw.fold()
    pwf, pbf = m.project.fold()
    return ew, eb, dwf[:, 0], dbf, pwf[:, :, 0, 0], pbf


_TILES = [(8, 16), (4, 16), (11, 11), (5, 11), (8, 13), (5, 13), (16, 16), (11, 22)]


def _tile_candidates(OH: int, OW: int, CinP: int, stride: int, dil: int,
                     expand: bool = True) -> List[Tuple[int, int]]:
    """2-D output tiles for the general fused-IR kernel: at most 8 MFMA pixel groups,
    LDS within one CU's 160 KB, and at most 25 % of the tiled area wasted."""
    out = []
    for ty, tx in _TILES:
        if -(-ty * tx // 16) > 8 or K.fused_ir_tile_lds(CinP, stride, dil, ty, tx, expand) > 160 * 1024:
            continue
        covered = -(-OH // ty) * ty * -(-OW // tx) * tx
        if covered <= 1.25 * OH * OW:
            out.append((ty, tx))
    return out


_PW_CONFIGS = [(2, 1), (2, 2), (2, 3), (4, 3), (4, 5)]


def pw_choice(name: str, gemm_op: Callable, x: torch.Tensor, w: torch.Tensor, b: torch.Tensor,
              out: torch.Tensor, *, M: int, Cin: int, Cout: int, ldo: Optional[int] = None,
              co_off: int = 0, act=None, N_out: Optional[int] = None) -> Callable:
    """A 1x1 conv step: the generic implicit GEMM (``gemm_op``) or the weight-streamed
    pw_conv kernel in a few (pixels-per-wave, chunks-per-workgroup) shapes, picked by
    the plan autotuner on the real buffers. Falls back to ``gemm_op`` alone when
    pw_conv has no instantiation for (Cin, Cout)."""
    Np = max(Cout, N_out or Cout)
    if not K.pw_supported(Cin, Np) or (ldo or Np) % 8 or co_off % 8:
        return gemm_op
    wpk = K.pack_pw_weights(w, b, N_out=Np)
    variants = [("gemm", [gemm_op])]
    NC = -(-Np // 64)
    for mt, nch in _PW_CONFIGS:
        if nch > NC:
            continue
        variants.append((f"pw{mt}x{nch}", [
            lambda *_, mt=mt, nch=nch: K.pw_conv(x, wpk, out, M=M, K=Cin, N=Np, ldo=ldo,
                                                  co_off=co_off, act=act, mt=mt, nch=nch)]))
    return Choice(name, variants)


def _dwp_rows_fit(ty: int, stages: int, dil: int, OW: int, cout: int) -> bool:
    """dw_proj_rows tile (ty rows x OW, <= 16 waves) and its LDS ring fit the CU."""
    nw = -(-ty * OW // 16)
    if nw > 16:
        return False
    halo = -(-(ty + 2 * dil) * (OW + 2 * dil) // 64) * 64  # octet planes of 64-pixel DMA pieces
    return (halo // 16 <= 4 * nw and
            stages * (halo * 64 + (cout // 16 + 1) * 1024) <= 160 * 1024)


def _rows_per_band(work: int, OH: int, targets) -> List[int]:
    return list(dict.fromkeys(min(max(2, -(-work // target)), OH) for target in targets))


class HipDeepLab(HipPlanModel):
    def __init__(self, model: DeepLabV3, device: torch.device, cfg=None):
        super().__init__(model, device, cfg.input_size if cfg is not None else 513,
                         confidence=bool(getattr(cfg, "serve_confidence", False)))
        dev = device
        bb = model.backbone
        self.kind = "mnv2" if isinstance(bb, MobileNetV2Backbone) else "resnet50"
        self.stem = _pack_stem(bb.stem, dev) + (bb.stem.k, bb.stem.stride, bb.stem.act, bb.stem.cout)
        self.blocks: List[dict] = []
        self.stem_block0 = None
        if self.kind == "mnv2":
            self.blocks = [self._pack_mnv2_block(blk, dev) for blk in bb.blocks]
            b0 = bb.blocks[0]
            s0 = b0.spec
            if (b0.expand is None and s0.stride == 1 and s0.dilation == 1 and s0.cin == 32 and
                    s0.cout == 16 and bb.stem.cout == 32 and bb.stem.k == 3 and bb.stem.stride == 2
                    and bb.stem.act == "relu6"):
                self.stem_block0 = K.pack_stem_block0(bb.stem, *_fold_block(b0)[2:], dev)
        else:
            for blk in bb.blocks:
                self.blocks.append(dict(
                    blk=blk,
                    conv1=_pack_dense(blk.conv1, dev), conv2=_pack_dense(blk.conv2, dev),
                    conv3=_pack_dense(blk.conv3, dev),
                    down=_pack_dense(blk.down, dev) if blk.down is not None else None))
        aspp = model.aspp
        self.aspp_c = aspp.cout
        self.aspp_b0 = _pack_dense(aspp.b0, dev)
        self.aspp_atrous = [(_pack_dense(b, dev), b.dilation) for b in aspp.atrous]
        self.cat_c = (1 + len(aspp.atrous)) * aspp.cout  # the spatial branches
        pw, pb = aspp.project.fold()  # [256, nb*256, 1, 1]
        pw = pw[:, :, 0, 0]
        self.proj_w = pw[:, : self.cat_c].contiguous().to(dev, torch.bfloat16)
        self.proj_b = pb.to(dev, torch.float32)
        self.has_pool = aspp.pool is not None
        if self.has_pool:
            qw, qb = aspp.pool.fold()
            self.pool_w = qw[:, :, 0, 0].contiguous().to(dev, torch.float32)
            self.pool_b = qb.to(dev, torch.float32)
            self.proj_pool_w = pw[:, self.cat_c:].contiguous().to(dev, torch.float32)
        lw, lb = model.logits.fold()
        self.logit_w = lw[:, :, 0, 0].reshape(lw.shape[0], 1, 1, -1).contiguous().to(dev, torch.bfloat16)
        self.logit_b = lb.to(dev, torch.float32)
        self.head = None  # aspp_head packed operands (built with the first plan)
        self._side_streams: List[torch.cuda.Stream] = []  # SSA_POOL_FORK side streams (one per plan)
        self._span_tables: Dict[tuple, dict] = {}

    @staticmethod
    def _pack_mnv2_block(blk, dev) -> dict:
        s = blk.spec
        d = dict(
            spec=s, module=blk,
            expand=_pack_dense(blk.expand, dev) if blk.expand is not None else None,
            dw=_pack_dw(blk.dw, dev),
            project=_pack_dense(blk.project, dev))
        row_ok = s.dilation == 1 and s.cin <= 64 and s.cout <= 96 and s.cin % 8 == 0
        shape = (-(-s.cout // 16), -(-s.cin // 32))
        tile_ok = s.cin % 8 == 0 and (
            shape in K.FUSED_TILE_SHAPES if blk.expand is not None
            else shape in K.FUSED_TILE_SHAPES_NOEXP and not s.residual)
        fold = _fold_block(blk)
        if row_ok or tile_ok:
            packed = K.pack_fused_ir(*fold, Cin=s.cin, hid=s.hidden, Cout=s.cout, stride=s.stride,
                                     residual=s.residual, device=dev, dil=s.dilation)
            if row_ok:
                d["fused"] = packed
            if tile_ok:
                d["fused_tile"] = packed
        if s.hidden % 32 == 0 and blk.expand is not None and not row_ok:
            d["dwproj"] = K.pack_project_padded(fold[4], fold[5], s.cout, s.hidden, dev)
        return d

    # ------------------------------------------------------------------ plan
    def _build(self, B: int, Hc: int, Wc: int, buf, bufs):
        mnv2 = self.kind == "mnv2"
        self._cam = (Hc, Wc)
        ops, st = (self._stem_mnv2 if mnv2 else self._stem_resnet)(B, Hc, Wc, buf, bufs)
        first = 1 if mnv2 and self.stem_block0 is not None else 0  # block 0 is in the stem choice
        for i in range(first, len(self.blocks)):
            bops, st = (self._mnv2_block if mnv2 else self._resnet_block)(buf, i, self.blocks[i], B, *st)
            ops += bops
        cat = buf("aspp_cat", B, st[1], st[2], self.cat_c)
        fork, pool, img_bias, item = self._aspp_pool(B, buf, bufs, *st)
        # (SSA_POOL_FORK: the pooling branch forks before the branch GEMMs and joins before the head)
        # (item: the pooling operands where it may run as work items of the grouped branch
        # GEMM; aspp.branches then covers the pooling steps too, in every variant)
        ops += fork + self._aspp_branches(B, buf, bufs, cat, *st, pool=pool, item=item)
        head, logits = self._head(B, buf, cat, img_bias, st[1], st[2])
        return ops + head + self._upsample(B, buf, logits, st[1], st[2])

    def _stem_op(self, B, Hc, Wc, buf, bufs):
        H, W = self.H, self.W
        sw, sb, sk, ss, sact, sc = self.stem
        OH, OW = conv_out_hw(H, W, sk, ss, 1)
        x = buf("stem", B, OH, OW, sc)
        bufs["_in_shape"] = torch.tensor([B, Hc, Wc])
        return (lambda frames, lx, ly: K.stem_conv(
            frames, lx, ly, sw, sb, x, H=H, W=W, OH=OH, OW=OW, Cout=sc, k=sk, stride=ss,
            act=sact)), (x, OH, OW, sc)

    def _stem_resnet(self, B, Hc, Wc, buf, bufs):
        """The ``stem`` choice (where the MFMA stem applies) and the max pool."""
        (sw, sb, sk, ss, sact, sc), H, W = self.stem, self.H, self.W
        stem, (x, h, w, c) = self._stem_op(B, Hc, Wc, buf, bufs)
        if (sc, sk) == (64, 7):
            # the dense 7x7 stem on bf16 MFMA, one wave per 16 channels (config 4 bf16:
            # 792 -> 127 us per 8 frames against the fp32 per-lane kernel, r8k)
            wpk = K.pack_stem_mfma(sw, sk, sc)
            bufs["const_stem_wpk"] = wpk
            stem = Choice("stem", [("fp32", [stem])] + [(f"mfmaw{tile[0]}x{tile[1]}", [
                lambda frames, lx, ly, tile=tile: K.stem_mfma(
                    frames, lx, ly, wpk, sb, x, H=H, W=W, OH=h, OW=w, Cout=sc, k=sk, stride=ss,
                    act=sact, tile=tile, per_wave=True)]) for tile in ((16, 32), (32, 32))])
        PH, PW = conv_out_hw(h, w, 3, 2, 1)
        y = buf("pool0", B, PH, PW, c)
        pool = (lambda *_: K.maxpool3x3s2(x, y, B=B, IH=h, IW=w, C=c, OH=PH, OW=PW))
        return [stem, pool], (y, PH, PW, c)

    def _stem_mnv2(self, B, Hc, Wc, buf, bufs):
        """The stem conv, or the ``stem+block0`` choice: stem + block 0 as one kernel (the
        257^2 x 32 stem tensor never hits HBM) against the two separate steps."""
        H, W = self.H, self.W
        stem, st = self._stem_op(B, Hc, Wc, buf, bufs)
        if self.stem_block0 is None:
            return [stem], st
        block0, st0 = self._mnv2_block(buf, 0, self.blocks[0], B, *st)
        sbp, out0, SH = self.stem_block0, st0[0], st[1]
        tiles = [(f"stem_block0_{ty}x{tx}", [
            lambda frames, lx, ly, ty=ty, tx=tx: K.stem_block0(
                frames, lx, ly, sbp, out0, H=H, W=W, tile=(ty, tx))])
            for ty, tx in ((8, 16), (4, 16), (8, 8), (16, 16), (8, 32), (12, 16))]
        # row-streaming bands: every input pixel gathered once, every stem pixel
        # computed once (stem_band.hip); bit-identical to the tile kernel
        bands: Dict[str, List[Callable]] = {}
        # band heights: grids of ~1-4 workgroups per CU, plus the heights whose
        # band count fills whole residency rounds (~3 of these 4-wave workgroups
        # fit a CU: a grid of 1.46 rounds pays a half-empty second round)
        for nbx in (3, 4, 5):
            Rs = [max(2, -(-B * nbx * SH // target)) for target in (256, 512, 1024)]
            Rs += [max(2, -(-SH // nby)) for nby in range(2, 13)
                   if B * nbx * nby in range(640, 800) or B * nbx * nby in range(1400, 1560)]
            for R in dict.fromkeys(Rs):
                for oneb in (True, False):
                    bands.setdefault(f"stem_band{R}x{nbx}" + ("" if oneb else "b2"), [
                        lambda frames, lx, ly, R=R, nbx=nbx, oneb=oneb: K.stem_band(
                            frames, lx, ly, sbp, out0, H=H, W=W, R=R, nbx=nbx, one_barrier=oneb,
                            row_repeat=self._row_repeat(0, SH, R))])
        # fixed order (pick 0 is the default, the tune file names variants): last band first
        return [Choice("stem+block0", list(bands.items())[::-1] + tiles +
                       [("separate", [stem] + block0)])], st0

    def _aspp_branches(self, B, buf, bufs, cat, x, h, w, c, pool=(), item=None):
        """The 1x1 and the atrous branches into their channel slices of ``cat``: one step
        per branch, or the ``aspp.branches`` choice of grouped launches against them, then
        the pooling steps ``pool``. With ``item`` (the pooling operands) the choice covers
        branches AND pooling: every variant carries the pooling work it implies, so each is
        timed with it -- the variants of before followed by ``pool``, and after them the
        ``grouped_v*+pool`` forms whose launch runs the pooling as work items of its grid."""
        pool = list(pool)
        A = self.aspp_c
        b0w, b0b = self.aspp_b0
        sep = [pw_choice("aspp.b0", lambda *_: K.conv_gemm(
            x, b0w, b0b, cat, B=B, IH=h, IW=w, Cin=c, OH=h, OW=w, Cout=A, k=1, ldo=self.cat_c,
            co_off=0, act="relu"), x, b0w, b0b, cat, M=B * h * w, Cin=c, Cout=A, ldo=self.cat_c,
            co_off=0, act="relu")]
        for j, ((aw, ab), rate) in enumerate(self.aspp_atrous):
            # atrous branch: raster-order tiles, or tiles grouped by tap validity
            # (tap_group_perm) so the kernel skips every all-padding tap
            variants = []
            if c in K.TAP_CIN and A % 8 == 0:
                twp, tbp = K.pack_tap_weights(aw, ab)
                for name, grouped in (("tap", False), ("tapg", True)):
                    perm = K.tap_group_perm(B, h, w, 3, rate, 256, self.device) if grouped else None
                    variants.append((name, [
                        lambda *_, twp=twp, tbp=tbp, rate=rate, j=j, perm=perm:
                        K.tap_conv(x, twp, tbp, cat, B=B, H=h, W=w, Cin=c, Cout=A, k=3, dil=rate,
                                   ldo=self.cat_c, co_off=(j + 1) * A, act="relu", perm=perm)]))
            for name, variant, bm in (("v4", 4, 0), ("v4g", 4, 128), ("v5g", 5, 128),
                                      ("v6g", 6, 256)):
                perm = K.tap_group_perm(B, h, w, 3, rate, bm, self.device) if bm else None
                variants.append((name, [
                    lambda *_, aw=aw, ab=ab, rate=rate, j=j, variant=variant, perm=perm: K.conv_gemm(
                        x, aw, ab, cat, B=B, IH=h, IW=w, Cin=c, OH=h, OW=w, Cout=A, k=3, dil=rate,
                        ldo=self.cat_c, co_off=(j + 1) * A, act="relu", variant=variant,
                        perm=perm)]))
            sep.append(Choice(f"aspp.rate{rate}", variants))
        if len(self.aspp_atrous) <= 3 and c % 8 == 0:
            grouped, fused = self._aspp_grouped(B, buf, bufs, cat, x, h, w, c, item)
            if not fused:
                return [Choice("aspp.branches", grouped + [("separate", sep)])] + pool
            return [Choice("aspp.branches", [(n, v + pool) for n, v in grouped] +
                           [("separate", sep + pool)] + fused)]
        return sep + pool

    def _aspp_grouped(self, B, buf, bufs, cat, x, h, w, c, item=None):
        """All spatial branches (1x1 + atrous) in ONE LPT-ordered LDS-DMA grid
        (conv_gemm_grouped), per tile shape and split-K factor. Returns (variants, the same
        launches with the pooling branch ``item`` as work items of the grid: ``name+pool``)."""
        A, dev = self.aspp_c, self.device
        b0w, b0b = self.aspp_b0
        grouped, fused = [], []

        def add(name, convs, order, gv, **kw):
            grouped.append((name, [lambda *_: K.conv_gemm_grouped(convs, order, gv, **kw)]))
            if item is not None and gv in K.GROUP_POOL_VARIANTS and K.pool_item_fits(gv, item["C"], item["N"]):
                order_p = K.with_pool_items(order, B)  # pool items first: never the tail
                bufs[f"aspp_order{name[len('grouped_v'):]}p"] = order_p
                fused.append((name + "+pool", [
                    lambda *_: K.conv_gemm_grouped(convs, order_p, gv, pool=item, **kw)]))
        # (variant 11, 128x128 tiles / 4 waves / 64 KiB LDS -- the only grouped variant
        # that fits two workgroups per CU -- gave label maps that differed in 26 of 450
        # runs with plan copies on three streams, every other variant 0 / 450:
        # profiles/r2_concurrency_race.txt; kept out until that is understood)
        # (branch-affine XCD orders, K.grouped_tile_order_branch, measured 6-16 us
        # slower on every variant: profiles/r3_negative_results.txt)
        for gv in (5, 6, 8, 12, 13, 14, 15, 16, 17, 18):
            BM = K.GROUP_TILE[gv][0]
            convs = [dict(x=x, w=b0w, bias=b0b, out=cat, B=B, IH=h, IW=w, Cin=c, OH=h, OW=w,
                          Cout=A, k=1, dil=1, ldo=self.cat_c, co_off=0, act="relu")]
            for j, ((aw, ab), rate) in enumerate(self.aspp_atrous):
                convs.append(dict(x=x, w=aw, bias=ab, out=cat, B=B, IH=h, IW=w, Cin=c, OH=h,
                                  OW=w, Cout=A, k=3, dil=rate, ldo=self.cat_c,
                                  co_off=(j + 1) * A, act="relu",
                                  perm=K.tap_group_perm(B, h, w, 3, rate, BM, dev)))
            order = K.grouped_tile_order(convs, gv, dev)
            bufs[f"aspp_order{gv}"] = order
            add(f"grouped_v{gv}", convs, order, gv)
            # small batches: split-K (a batch-1 grid is ~40 tiles of up to 45 K stages for
            # 256 CUs); fp32 partials + one combine (bias, ReLU) over the concat buffer
            ks_opts = (2, 4, 6) if B <= 2 else (2, 3) if B <= 8 else ()
            if ks_opts and gv in (5, 17, 18) and A * (len(self.aspp_atrous) + 1) == self.cat_c:
                if "aspp_part" not in bufs:
                    buf("aspp_part", max(ks_opts) * B * h * w * self.cat_c, dtype=torch.float32)
                    bufs["const_aspp_bias_cat"] = torch.cat(
                        [b0b.float()] + [ab.float() for (_, ab), _ in self.aspp_atrous]).to(dev).contiguous()
                ntile = max(-(-(cv["perm"].numel() if cv.get("perm") is not None else B * h * w) // BM)
                            for cv in convs) * -(-A // K.GROUP_TILE[gv][1])
                cnt = buf(f"aspp_cnt{gv}", 4 * ntile, dtype=torch.int32)
                for ks in ks_opts:
                    order_k = K.grouped_tile_order(convs, gv, dev, ks=ks)
                    bufs[f"aspp_order{gv}k{ks}"] = order_k
                    for inl in (False, True):  # in-launch combine by each tile's last K slice
                        add(f"grouped_v{gv}k{ks}" + ("c" if inl else ""), convs, order_k, gv, ks=ks,
                            part=bufs["aspp_part"], bias_cat=bufs["const_aspp_bias_cat"],
                            cnt=cnt if inl else None)
        return grouped, fused

    def _aspp_pool(self, B, buf, bufs, x, h, w, c):
        """The image-pooling branch -> per-image bias of the projection. Returns (ops to run
        before the branches, ops to run before the head, img_bias, the operands for running
        it as work items of the grouped branch GEMM -- or None where that form is not offered:
        SSA_POOL_FUSED=0, the side-stream fork, the matvec fall-back shapes)."""
        if not self.has_pool:
            return [], [], None, None
        A, dev = self.aspp_c, self.device
        img_bias = buf("img_bias", B, A, dtype=torch.float32)
        gws = K.gap_workspace(B, c, dev)
        bufs["gap_ws"] = gws
        if not (c <= 2048 and A <= 512 and c % 8 == 0 and A % 4 == 0):
            gap = buf("gap", B, c, dtype=torch.float32)
            pooled = buf("pooled", B, A, dtype=torch.float32)
            return [], [
                lambda *_: K.global_avgpool(x, gap, B=B, HW=h * w, C=c, ws=gws),
                lambda *_: K.matvec(gap, self.pool_w, self.pool_b, pooled, B=B, N=A, K=c, act="relu"),
                lambda *_: K.matvec(pooled, self.proj_pool_w, None, img_bias, B=B, N=A, K=A)], img_bias, None
        # GAP partials + one per-image kernel for the pooled MLP (aspp_pool)
        w1t = self.pool_w.t().contiguous()
        w2t = self.proj_pool_w.t().contiguous()
        bufs["pool_w1t"], bufs["pool_w2t"] = w1t, w2t
        pool_op = (lambda *_: K.aspp_pool(
            x, gws, w1t, self.pool_b, w2t, img_bias, B=B, HW=h * w, C=c, N=A))
        if not (os.environ.get("SSA_POOL_FORK", "0") == "1" and torch.cuda.is_available()):
            item = dict(x=x, w1t=w1t, b1=self.pool_b, w2t=w2t, img_bias=img_bias, B=B, HW=h * w, C=c, N=A)
            return [], [pool_op], img_bias, item if os.environ.get("SSA_POOL_FUSED", "1") != "0" else None
        # the pooling branch (GAP partials + per-image MLP: 32 + 32 small
        # workgroups, ~26 us of latency at B = 32) on a side stream forked before
        # the grouped branch GEMM and joined before the head: its few waves fit
        # beside the GEMM's 16 per CU instead of running after it (event fork /
        # join, captured into the hipGraph like the rest of the plan)
        side = torch.cuda.Stream(dev)
        ev_f, ev_j = torch.cuda.Event(), torch.cuda.Event()
        self._side_streams.append(side)

        def fork_op(*args):
            ev_f.record(torch.cuda.current_stream())
            side.wait_event(ev_f)
            with torch.cuda.stream(side):
                pool_op(*args)
            ev_j.record(side)

        return [fork_op], [lambda *_: torch.cuda.current_stream().wait_event(ev_j)], img_bias, None

    def _head(self, B, buf, cat, img_bias, h, w):
        """Projection and logits: two steps, or the ``aspp.head`` choice of the fused kernel
        against them. Returns (ops, logits buffer)."""
        A = self.aspp_c
        proj = buf("aspp_proj", B, h, w, A)
        proj_variants = [(f"v{v}", [
            lambda *_, v=v: K.conv_gemm(
                cat, self.proj_w, self.proj_b, proj, B=B, IH=h, IW=w, Cin=self.cat_c, OH=h, OW=w,
                Cout=A, k=1, act="relu", img_bias=img_bias, variant=v)]) for v in (4, 3, 5, 6)]
        logits = buf("logits", B, h, w, self.ldk)
        split = [Choice("aspp.proj", proj_variants), pw_choice("logits", lambda *_: K.conv_gemm(
            proj, self.logit_w, self.logit_b, logits, B=B, IH=h, IW=w, Cin=A, OH=h, OW=w,
            Cout=self.num_classes, k=1, ldo=self.ldk, act=None), proj, self.logit_w,
            self.logit_b, logits, M=B * h * w, Cin=A, Cout=self.num_classes, ldo=self.ldk, act=None,
            N_out=self.ldk)]
        if not (A == 256 and self.cat_c == 1024 and self.num_classes <= 32 and self.ldk <= 32):
            return split, logits
        # projection + bias + pooling bias + ReLU + logits in one kernel: the projection
        # stays on chip (aspp_head.hip), no vendor GEMM on the hot path
        if self.head is None:
            self.head = K.pack_aspp_head(self.proj_w, self.proj_b, self.logit_w, self.logit_b, self.device)
        Mh = B * h * w
        g0 = K.aspp_head_groups(Mh)
        head = [(f"head_g{g}" + ("w" if nw == 16 else ""), [lambda *_, g=g, nw=nw: K.aspp_head(
            cat.view(Mh, self.cat_c), self.head, logits.view(Mh, self.ldk), M=Mh, HW=h * w,
            ldo=self.ldk, img_bias=img_bias, G=g, waves=nw)]) for g in K.ASPP_HEAD_G
            if g == g0 or (g < g0 and -(-Mh // (16 * g)) <= 1024) for nw in (8, 16)]
        return [Choice("aspp.head", head + [("split", split)])], logits

    def _upsample(self, B, buf, logits, h, w):
        # upsample + argmax: row-block (LDS-staged, coalesced stores), per-lane stores, or
        # per-lane with wave-union class pruning; with confidence, the one two-plane kernel
        return self._final_op(buf, logits, B, h, w, ("rows", "lane", "union", "cand"))

    # ------------------------------------------------------- MobileNetV2 block
    def _mnv2_block(self, buf, i, blk, B, x, h, w, c):
        """Block ``i`` as the ``block{i}`` choice: the unfused steps (1x1 expansion,
        depthwise, 1x1 projection) and every fused kernel family that fits the block."""
        s = blk["spec"]
        hid = s.hidden
        unfused: List[Callable] = []
        e = x
        if blk["expand"] is not None:
            ew, eb = blk["expand"]
            e = buf(f"b{i}_exp", B, h, w, hid)
            unfused.append(pw_choice(f"block{i}.expand", lambda *_: K.conv_gemm(
                x, ew, eb, e, B=B, IH=h, IW=w, Cin=c, OH=h, OW=w, Cout=hid, k=1, act="relu6"),
                x, ew, eb, e, M=B * h * w, Cin=c, Cout=hid, act="relu6"))
        OH, OW = conv_out_hw(h, w, 3, s.stride, s.dilation)
        dw_w, dw_b = blk["dw"]
        d = buf(f"b{i}_dw", B, OH, OW, hid)
        unfused.append(lambda *_: K.depthwise3x3(
            e, dw_w, dw_b, d, B=B, IH=h, IW=w, C=hid, OH=OH, OW=OW, stride=s.stride,
            dil=s.dilation, act="relu6"))
        pw_, pb_ = blk["project"]
        out = buf(f"b{i}_out", B, OH, OW, s.cout)
        res = x if s.residual else None
        unfused.append(lambda *_: K.conv_gemm(
            d, pw_, pb_, out, B=B, IH=OH, IW=OW, Cin=hid, OH=OH, OW=OW, Cout=s.cout, k=1,
            act=None, res=res))
        g = SimpleNamespace(i=i, blk=blk, s=s, B=B, x=x, h=h, w=w, c=c, hid=hid, e=e, out=out,
                            res=res, OH=OH, OW=OW, buf=buf, expand_op=unfused[0])
        # the families allocate their buffers in this order; the variants are listed in the
        # order below, which is fixed: pick 0 is the default and the tune file names variants
        dwp, dwproj, tile = self._dwp_variants(g), self._dwproj_variants(g), self._tile_variants(g)
        stream, band, slices = self._stream_variants(g), self._band_variants(g), self._slice_variants(g)
        variants = slices + band + stream + tile + [("unfused", unfused)] + dwp + dwproj
        return [Choice(f"block{i}", variants)], (out, OH, OW, s.cout)

    def _dwp_variants(self, g):
        """``dwp*``: expansion (weight-streamed pw_conv, fp16 out) -> fused depthwise + projection."""
        s, blk, B, h, w, c, hid, OH, OW = g.s, g.blk, g.B, g.h, g.w, g.c, g.hid, g.OH, g.OW
        if not (blk["expand"] is not None and hid % 32 == 0 and s.cout in K.DWP_COUT
                and K.pw_supported(c, hid)):
            return []
        ew, eb = blk["expand"]
        (pw_, pb_), (dw_w, dw_b) = blk["project"], blk["dw"]
        e16 = g.buf(f"b{g.i}_exp16", B, h, w, hid, dtype=torch.float16)
        ewpk = K.pack_pw_weights(ew, eb)
        wpk_dp = K.pack_dw_proj(pw_[:, 0, 0, :], dw_w, dw_b)
        M = B * h * w
        cfgs = [("w", 4, 0, 2, False)]
        if s.stride == 1:
            cfgs += [("r", 4, ty, 2, False) for ty in (2, 3, 4)]
            cfgs += [("r", 4, ty, st, True) for ty in (2, 3, 4, 6) for st in (2, 3, 4)
                     if _dwp_rows_fit(ty, st, s.dilation, OW, s.cout)]
        out = []
        for mt, nch in ((2, 3),):
            for kind, nw, ty, st, xcd in cfgs:
                tag = f"dwp{kind}{nw if not ty else ty}" + (f"s{st}x" if xcd else "")
                out.append((f"{tag}.pw{mt}x{nch}", [
                    lambda *_, mt=mt, nch=nch: K.pw_conv(
                        g.x, ewpk, e16, M=M, K=c, N=hid, act="relu6", mt=mt, nch=nch),
                    lambda *_, nw=nw, ty=ty, st=st, xcd=xcd:
                    K.dw_proj_fused(e16, wpk_dp, pb_, g.out, B=B, IH=h, IW=w, hid=hid,
                                    Cout=s.cout, OH=OH, OW=OW, stride=s.stride,
                                    dil=s.dilation, res=g.res, waves=nw, rows=ty, stages=st,
                                    xcd=xcd)]))
        return out

    def _dwproj_variants(self, g):
        """``dwproj``: the unfused expansion step, then depthwise + projection in one kernel."""
        if "dwproj" not in g.blk:
            return []
        s, (dpw, dpb), (dw_w, dw_b) = g.s, g.blk["dwproj"], g.blk["dw"]
        return [("dwproj", [g.expand_op, lambda *_: K.dw_project(
            g.e, dw_w, dw_b, dpw, dpb, g.out, B=g.B, IH=g.h, IW=g.w, hid=g.hid, Cout=s.cout,
            OH=g.OH, OW=g.OW, stride=s.stride, dil=s.dilation, res=g.res)])]

    def _tile_variants(self, g):
        """``fused`` (row kernel) and ``tile*`` (2-D tiles): the whole block in one fused_ir launch."""
        s, blk = g.s, g.blk
        geom = dict(B=g.B, IH=g.h, IW=g.w, OH=g.OH, OW=g.OW)
        out = []
        if "fused_tile" in blk:
            fp = blk["fused_tile"]
            for tile in _tile_candidates(g.OH, g.OW, fp["CinP"], s.stride, s.dilation,
                                         fp["we"] is not None):
                out.append((f"tile{tile[0]}x{tile[1]}", [
                    lambda *_, fp=fp, tile=tile: K.fused_ir(g.x, fp, g.out, tile=tile, **geom)]))
        if "fused" in blk:
            out.append(("fused", [lambda *_, fp=blk["fused"]: K.fused_ir(g.x, fp, g.out, **geom)]))
        return out[::-1]  # the last one built is listed first (fixed order: _mnv2_block)

    def _stream_variants(self, g):
        """``stream*``: the expanded tensor kept on chip, raster spans of ~h*w/S pixels per
        workgroup (fused_ir_stream), on the raster or the phase-class lattice table."""
        s, blk, B, h, w = g.s, g.blk, g.B, g.h, g.w
        if not (blk["expand"] is not None and s.stride == 1 and (s.cin, s.cout) in FS.STREAM_SHAPES):
            return []
        narrow = s.cout <= 96 and s.dilation == 1
        out = []

        def stream(name, tab, v, **kw):
            sp = self._packed(blk, "span")
            out.append((name, [lambda *_: FS.fused_ir_stream(
                g.x, sp, tab, g.out, B=B, residual=s.residual, variant=v, **kw)]))

        for S in self._span_counts(B, h, w):
            if FS.stream_supported(s.cin, s.cout, 1, h, w, S, s.dilation, lattice=True):
                # dilation 2 on the phase-class lattice: halo +- 1 lattice row (ops/fused_span
                # .lattice_table), 3 halo rounds per expansion wave instead of 5
                ltab = self._span_table(h, w, S, s.dilation, lattice=True)
                for v in ((0, 1, 2, 4) if s.cout <= 160 else (1,)):
                    stream(f"stream{S}" + {0: "", 1: "g", 2: "w", 4: "r3"}[v] + "L", ltab, v)
                self._split_hidden(g, S, stream, ltab, [(0 if s.cout <= 160 else 1, "L")])
            if FS.stream_supported(s.cin, s.cout, 1, h, w, S, s.dilation):
                tab = self._span_table(h, w, S, s.dilation)
                # wave-specialised: expansion waves | depthwise+projection waves
                # 4 / 6: the 3-slot chunk ring (72 instead of 81 KiB for blocks 7-9: two
                # workgroups per CU)
                vs = ((0, 1, 2) if narrow else (0, 1)) + \
                    ((4,) if s.cout <= 160 else ()) + ((6,) if narrow else ())
                for v in vs:
                    stream(f"stream{S}" + {0: "", 1: "g", 2: "w", 4: "r3", 6: "wr3"}[v], tab, v)
                self._split_hidden(g, S, stream, tab, [(0, ""), (2, "w")] if narrow else [(0, "")])
        return out[::-1]  # the last one built is listed first (fixed order: _mnv2_block)

    @staticmethod
    def _split_hidden(g, S, stream, tab, kernels) -> None:
        """``stream{S}{tag}h{hs}[c]``, small batches: the hidden chunks of a span over hs
        workgroups (fp32 partials + stream_combine, or the in-launch combine "c"), so
        B * S * hs workgroups share the chip. ``kernels``: (variant, tag) pairs."""
        s, B, i = g.s, g.B, g.i
        nc = -(-g.hid // 32)
        hs_opts = [hs for hs in (2, 3, 4, 6) if hs <= nc and B * S * hs <= 512] if B <= 16 else []
        if not hs_opts:
            return
        if not hasattr(g, "part"):
            g.part = g.buf(f"b{i}_part", max(hs_opts) * B * g.h * g.w * s.cout, dtype=torch.float32)
        # per-span arrival tickets of the in-launch combine ("...c" variants)
        cnt = g.buf(f"b{i}_cnt{S}", B * S, dtype=torch.int32)
        for hs in hs_opts:
            for v, tag in kernels:
                for inl in (False, True):
                    stream(f"stream{S}{tag}h{hs}" + ("c" if inl else ""), tab, v, hsplit=hs,
                           part=g.part, cnt=cnt if inl else None)

    def _band_variants(self, g):
        """``band*``: row-streaming bands, every input row expanded once into an on-chip fp16 row."""
        s, blk, B, OH, OW = g.s, g.blk, g.B, g.OH, g.OW
        if not (blk["expand"] is not None and
                FB.band_supported(s.cin, g.hid, s.cout, s.stride, s.dilation, OW)):
            return []
        bp_ = self._packed(blk, "band")
        out = []
        # (split 2 -- blocks 1-2 as two column bands, 5+5 waves with hs 2 -- measured
        # 86-92 us vs 65-69 us for the full-width band: profiles/r3_negative_results.txt)
        for split in (1,):
            if not FB.band_supported(s.cin, g.hid, s.cout, s.stride, s.dilation, OW, split):
                continue
            for hs in ((1, 2) if FB.band_waves(OW, split) <= 8 else (1,)):
                for nslot in (2, 1):
                    if FB.band_lds(bp_, s.stride, OW, nslot, hs, split) > 160 * 1024:
                        continue
                    # rows per band: grids of ~1-4 workgroups per CU slot (2 per CU x 256 CUs);
                    # fewer rows re-expand more halo rows, more rows fill fewer CUs
                    for R in _rows_per_band(B * OH, OH, (256, 512, 1024)):
                        tag = f"band{R}s{nslot}" + ("h" if hs == 2 else "") + ("c" if split == 2 else "")
                        out.append((tag, [
                            lambda *_, R=R, nslot=nslot, hs=hs, split=split: FB.fused_ir_band(
                                g.x, bp_, g.out, B=B, IH=g.h, IW=g.w, stride=s.stride,
                                residual=s.residual, R=R, nslot=nslot, hs=hs, split=split)]))
        return out[::-1]  # the last one built is listed first (fixed order: _mnv2_block)

    def _slice_variants(self, g):
        """``slice*``: hidden-sliced row streaming, wave = column group x 32 hidden channels,
        the chunk's weights in VGPRs (fused_ir_slice.hip: the band kernel's LDS weight
        re-reads were its bottleneck)."""
        s, blk, B, OH, OW = g.s, g.blk, g.B, g.OH, g.OW
        if blk["expand"] is None:
            return []
        out = []
        # the letterbox's constant rows computed once: the kernel derives them from the
        # LUT of the call and this block's receptive field (ops/row_repeat.py); per launch,
        # where _row_repeat expects it to pay
        rf = self._block_rf(g.i)
        for nw in FB.slice_widths(s.cin, g.hid, s.cout, s.stride, s.dilation):
            bp_ = self._packed(blk, "band")
            twmax = 16 * nw - (2 if s.stride == 1 else 1)
            nbx = -(-OW // twmax)
            for oneb in (False, True):  # "o": one barrier per input row
                if FB.slice_lds(bp_, s.stride, OW, nw, oneb) > 160 * 1024:
                    continue
                # rows per band (one 12-15-wave workgroup per CU): grids of ~1, 2, 3 and 4
                # workgroups per CU (256 CUs)
                for R in _rows_per_band(B * nbx * OH, OH, (256, 512, 768, 1024)):
                    out.append((f"slice{R}w{nw}" + ("o" if oneb else ""), [
                        lambda frames, lx, ly, R=R, nw=nw, bp_=bp_, oneb=oneb,
                        rr=self._row_repeat(g.i, OH, R, s.stride): FB.fused_ir_slice(
                            g.x, bp_, g.out, B=B, IH=g.h, IW=g.w, stride=s.stride,
                            residual=s.residual, R=R, nw=nw, one_barrier=oneb,
                            lut_y=ly if rr else None, H=self.H, rf=rf)]))
        return out[::-1]  # the last one built is listed first (fixed order: _mnv2_block)

    def _row_repeat(self, i: int, OH: int, R: int, stride: int = 2) -> bool:
        """Whether a row-streaming launch of block ``i`` (0: stem + block 0) with bands of
        ``R`` of its ``OH`` rows gets the row repeat. The kernel derives the zone from the LUT
        of the call; this only decides where finding it is worth its cost, from the
        letterbox of the plan's camera: on where a band gets shorter (a square or portrait
        camera, or block 6's 2 of 33 rows at 4:3, would pay the LUT scan for nothing), and
        in the stride-2 slice blocks only: the stride-1 blocks' time is mostly per-workgroup
        fixed cost, and block 2 measured no faster with 4 of 17 rows fewer.
        ``SSA_ROW_REPEAT=all`` turns it on everywhere (tests), ``0`` off."""
        m, rf = RR.mode(), self._block_rf(i)
        if m == "off" or rf is None:
            return False
        if m == "all":
            return True
        from ..ops import reference_ops as R_
        Hc, Wc = self._cam
        p0 = RR.pad_start(R_.letterbox_luts(Wc, Hc, self.W, self.H)[1])
        return stride == 2 and RR.pays(p0, self.H, OH, R, rf)

    def _block_rf(self, i: int) -> Optional[Tuple[int, int, int]]:
        """The cumulative vertical receptive field of block ``i``'s output rows in
        model-input rows (ops/row_repeat.py), None where the 3x3 pad-1 chain does not hold."""
        sk, ss = self.stem[2], self.stem[3]
        if sk != 3:
            return None
        rf = RR.rf_conv3x3(RR.RF_INPUT, ss)
        for blk in self.blocks[:i + 1]:
            rf = RR.rf_conv3x3(rf, blk["spec"].stride, blk["spec"].dilation)
        return rf

    def _packed(self, blk: dict, key: str) -> dict:
        """The block's weights in the "span" / "band" kernels' layout, packed on first use."""
        if key not in blk:
            s, pack = blk["spec"], FS.pack_fused_span if key == "span" else FB.pack_fused_band
            blk[key] = pack(*_fold_block(blk["module"]), Cin=s.cin, hid=s.hidden, Cout=s.cout,
                            device=self.device)
        return blk[key]

    @staticmethod
    def _span_counts(B: int, h: int, w: int) -> List[int]:
        """Spans per image for the fused span kernel: the smallest count whose spans fit
        the kernel's 144 pixels, and 2x / 4x that for small batches (more workgroups)."""
        s0 = -(-h * w // (FS.MAX_GROUPS * 16))
        return [s0, 2 * s0] + ([4 * s0] if B * s0 < 256 else [])

    def _span_table(self, h: int, w: int, S: int, dil: int, lattice: bool = False):
        key = (h, w, S, dil, lattice)
        if key not in self._span_tables:
            self._span_tables[key] = (FS.lattice_table if lattice else FS.span_table)(h, w, S, dil, self.device)
        return self._span_tables[key]

    # ------------------------------------------------------------ ResNet block
    def _resnet_block(self, buf, i, blk, B, x, h, w, c):
        m = blk["blk"]
        width, cout = m.conv1.cout, m.conv3.cout
        ops: List[Callable] = []
        w1, b1 = blk["conv1"]
        t1 = buf(f"r{i}_c1", B, h, w, width)
        ops.append(lambda *_: K.conv_gemm(
            x, w1, b1, t1, B=B, IH=h, IW=w, Cin=c, OH=h, OW=w, Cout=width, k=1, act="relu"))
        OH, OW = conv_out_hw(h, w, 3, m.stride, m.dilation)
        w2, b2 = blk["conv2"]
        t2 = buf(f"r{i}_c2", B, OH, OW, width)
        ops.append(lambda *_: K.conv_gemm(
            t1, w2, b2, t2, B=B, IH=h, IW=w, Cin=width, OH=OH, OW=OW, Cout=width, k=3,
            stride=m.stride, dil=m.dilation, act="relu"))
        if blk["down"] is not None:
            wd, bd = blk["down"]
            idt = buf(f"r{i}_down", B, OH, OW, cout)
            ops.append(lambda *_: K.conv_gemm(
                x, wd, bd, idt, B=B, IH=h, IW=w, Cin=c, OH=OH, OW=OW, Cout=cout, k=1,
                stride=m.stride, act=None))
        else:
            idt = x
        w3, b3 = blk["conv3"]
        out = buf(f"r{i}_out", B, OH, OW, cout)
        ops.append(lambda *_: K.conv_gemm(
            t2, w3, b3, out, B=B, IH=OH, IW=OW, Cin=width, OH=OH, OW=OW, Cout=cout, k=1,
            act="relu", res=idt))
        return ops, (out, OH, OW, cout)
