"""The float64 reference of the upsample + argmax kernels and the guarded label plane, shared
by tests/test_confidence_gpu.py (``upsample_argmax_conf``) and tests/test_hip_kernels.py
(``upsample_argmax``, every variant and dispatch branch).

The rule both use: a label must equal the float64 argmax of the float64 bilinear interpolant
(align_corners) at every pixel whose float64 top-two margin exceeds MARGIN. The kernels' three
fp32 lerps err by < 8e-6 for |logit| <= 32, so MARGIN is over 10 x the interpolation error;
a test's inputs must leave at most MAX_UNDECIDED of the map below it.
"""
import numpy as np
import torch
import torch.nn.functional as F

DEV = "cuda"
GUARD = 0xEE
MARGIN = 1e-4
MAX_UNDECIDED = 0.002


def ref64(logits, K, H, W):
    """(255 * p64, float64 argmax, top-two margin) of NHWC bf16 logits."""
    u = F.interpolate(logits[..., :K].double().permute(0, 3, 1, 2), size=(H, W), mode="bilinear",
                      align_corners=True)
    p = torch.softmax(u, 1).amax(1)
    top2 = u.topk(2, dim=1).values
    return 255.0 * p, u.argmax(1), top2[:, 0] - top2[:, 1]


def label_ref(logits, K, H, W, without=None, margin=MARGIN):
    """(float64 argmax, mask of the pixels whose top-two margin exceeds ``margin``), on the device
    of ``logits`` (the float64 interpolant of a 2 x 1025 x 1025 x 19 map is 320 MB: the device
    tests compute it there). ``without``: a class left out of the contest. ``margin``: MARGIN
    presumes |logit| <= 32; larger logits scale it (tests/plan_bound.py)."""
    u = F.interpolate(logits[..., :K].double().permute(0, 3, 1, 2), size=(H, W), mode="bilinear",
                      align_corners=True)
    if without is not None:
        u[:, without] = -1e30
    if K == 1:
        return u.argmax(1), torch.ones_like(u[:, 0], dtype=torch.bool)
    top2 = u.topk(2, dim=1).values
    return u.argmax(1), (top2[:, 0] - top2[:, 1]) > margin


def guarded(B, H, W):
    """A contiguous (B, H, W) uint8 plane with one guard row of 0xEE before and after."""
    raw = torch.full((B * H + 2, W), GUARD, dtype=torch.uint8, device=DEV)
    return raw, raw[1:-1].view(B, H, W)


def make_logits(B, h, w, K, ldk, field, seed=7):
    """NHWC bf16 logits. ``noise``: i.i.d. normal; ``smooth``: a coarse random field upsampled
    to h x w (large regions); ``zeros``; ``perm``: integer scores, distinct integers of
    -16 .. 16 (-31 .. 31 for more than 33 channels) at every source pixel (no two classes tie at a source pixel, which bf16 noise does
    at about 1 % of them); ``twins``: the same with class ``TWIN[1]`` an exact copy of class
    ``TWIN[0]``. Integer scores tie exactly wherever the lerp weights are simple fractions
    (9 -> 65 has weights k / 8), so their tests use output sizes such as 67 x 71. The padding
    channels K .. ldk hold +100: one of them in the maximum is an error."""
    g = torch.Generator().manual_seed(seed)
    if field == "noise":
        x = torch.randn(B, h, w, ldk, generator=g)
    elif field == "smooth":
        coarse = torch.randn(B, ldk, 4, 4, generator=g) * 4
        x = F.interpolate(coarse, size=(h, w), mode="bilinear", align_corners=True).permute(0, 2, 3, 1)
    elif field == "zeros":
        x = torch.zeros(B, h, w, ldk)
    else:
        # |score| <= 16 where a tagged variant can run (K <= 32): its tags move a score by up to
        # 32 fp32 ulps, 3e-5 below 16, and two such moves must stay inside MARGIN
        r = 16 if ldk <= 33 else 31
        assert ldk <= 2 * r + 1
        x = torch.rand(B, h, w, 2 * r + 1, generator=g).argsort(-1)[..., :ldk].float() - float(r)
        if field == "twins":
            x[..., TWIN[1]] = x[..., TWIN[0]]
        else:
            assert field == "perm"
    x = x.contiguous().to(torch.bfloat16)
    x[..., K:] = 100.0
    return x


TWIN = (2, 5)


def upsample_path(B, h, w, H, W, K, ldk, variant):
    """The kernel ``ops.hip_ops.upsample_argmax`` runs, by the dispatch arithmetic of
    csrc/hip/model_ops.hip (fp32 scale): the variant after demotion, or 5 for the direct
    (per-pixel gather) kernel."""
    sw = np.float32(w - 1) / np.float32(W - 1) if W > 1 else np.float32(0)
    interval = (K <= 32 and ldk % 8 == 0 and ldk >= (24 if K <= 24 else 32) and w >= 2 and W > 1 and
                sw > 0 and np.float32(1) / sw <= np.float32(30) and B * H * w < 2 ** 31)
    variant = variant or 1
    if interval and variant in (3, 4) and (w > 256 or (256 // w) * W > 65536):
        variant -= 2
    return variant if interval and variant != 5 else 5


SQUARE_SHAPES = [(33, 513, 21), (65, 1025, 19), (9, 65, 21), (33, 257, 30)]  # h, H, K (B = 2, ldk = K up to 8)

# B, h, w, H, W, K, ldk, the kernel the dispatch must choose
UPSAMPLE_SHAPES = [
    (2, 9, 17, 65, 129, 21, 24, "interval"),  # non-square
    (2, 17, 9, 129, 65, 21, 24, "interval"),
    (1, 9, 9, 65, 65, 21, 24, "interval"),    # batch 1
    (3, 9, 9, 65, 65, 19, 24, "interval"),    # 195 rows in blocks of 256 / 9 = 28: last block partial, odd W
    (2, 9, 9, 65, 65, 8, 24, "interval"),     # runtime K of the <24, 0> kernels
    (2, 9, 9, 65, 65, 24, 24, "interval"),
    (2, 9, 9, 65, 65, 32, 32, "interval"),    # the class-count edge
    (2, 9, 9, 65, 65, 21, 32, "interval"),    # ldk 32: eleven padding channels at +100
    # downsampling: sw = 2, every odd source interval empty. Every output pixel IS a source pixel,
    # and bf16 noise ties its top two classes at 1 % of them: distinct integer scores instead
    (2, 33, 33, 17, 17, 21, 24, "interval", ("perm",)),
    (2, 5, 5, 40, 40, 40, 40, "direct"),      # K > 32
    (2, 9, 9, 65, 65, 21, 21, "direct"),      # ldk % 8 != 0
    (2, 9, 9, 65, 65, 8, 8, "direct"),        # rows shorter than the 24 channels the interval load reads
    (2, 3, 3, 65, 65, 21, 24, "direct"),      # 1 / sw = 32 > 30
    (2, 9, 3, 65, 1, 21, 24, "direct", ("smooth",)),  # W = 1 (130 pixels: one near-tie of the noise is 0.8 %)
    (2, 9, 1, 65, 9, 21, 24, "direct"),       # w = 1
    # The row-block variants 3 / 4 are demoted to 1 / 2 when w > 256 or (256 / w) W > 65536.
    # Under 1 / sw <= 30, W <= 30 w - 29, so (256 / w) W < 7680: only w > 256 can demote.
    (1, 2, 257, 3, 300, 21, 24, "demoted"),
]

TIE_SHAPES = [  # output sizes whose lerp weights are no simple fractions (``make_logits``)
    (2, 9, 9, 67, 71, 21, 24, "interval"),
    (3, 9, 9, 67, 71, 19, 24, "interval"),   # 201 rows in blocks of 28
    (2, 9, 9, 67, 71, 24, 24, "interval"),   # runtime K
    (2, 9, 9, 67, 71, 32, 32, "interval"),
    (2, 5, 5, 40, 40, 40, 40, "direct"),
    (1, 2, 257, 3, 300, 21, 24, "demoted"),
]


def square_logits(h, K, field):
    """The inputs of test_upsample_argmax (B = 2, h x h, channels past K random as well)."""
    g = torch.Generator().manual_seed(7)
    ldk = (K + 7) // 8 * 8
    if field == "noise":
        return torch.randn(2, h, h, ldk, generator=g).to(torch.bfloat16)
    coarse = torch.randn(2, ldk, 4, 4, generator=g) * 4
    return F.interpolate(coarse, size=(h, h), mode="bilinear", align_corners=True) \
        .permute(0, 2, 3, 1).contiguous().to(torch.bfloat16)


def branch_inputs():
    """(id, logits, K, H, W, class left out) of every input of the device tests of
    ``upsample_argmax``: the square maps, every dispatch branch, the twins of the tie cases."""
    for h, H, K in SQUARE_SHAPES:
        for field in ("noise", "smooth"):
            yield f"square-{h}-{H}-{K}-{field}", (lambda h=h, K=K, field=field: square_logits(h, K, field)), K, H, H, None
    for s in UPSAMPLE_SHAPES:
        B, h, w, H, W, K, ldk = s[:7]
        for field in (s[8] if len(s) > 8 else ("noise", "smooth")):
            yield ("-".join(map(str, s[:7])) + "-" + field,
                   (lambda B=B, h=h, w=w, K=K, ldk=ldk, field=field: make_logits(B, h, w, K, ldk, field)), K, H, W, None)
    for B, h, w, H, W, K, ldk, _ in TIE_SHAPES:
        yield (f"{B}-{h}-{w}-{H}-{W}-{K}-{ldk}-twins",
               (lambda B=B, h=h, w=w, K=K, ldk=ldk: make_logits(B, h, w, K, ldk, "twins")), K, H, W, TWIN[1])
