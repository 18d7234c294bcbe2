"""The inputs of the device tests of ``upsample_argmax`` (tests/upsample_ref.py), judged on the
CPU from the float64 reference alone: every one leaves at most MAX_UNDECIDED of its pixels
below the top-two margin, so the margin rule decides nearly the whole map, and the twins of
the tie cases are exact copies. The device tests assert the same share before they compare.
"""
import pytest
import torch

import upsample_ref as UR

INPUTS = list(UR.branch_inputs())


def _undecided(logits, K, H, W, without):
    """Share of the pixels below the margin; one image at a time (the float64 interpolant of
    a 1025 x 1025 x 19 map is 160 MB)."""
    below = total = 0
    for img in logits:
        _, decided = UR.label_ref(img[None], K, H, W, without=without)
        below += int((~decided).sum())
        total += decided.numel()
    return below / total


@pytest.mark.parametrize("make,K,H,W,without", [i[1:] for i in INPUTS], ids=[i[0] for i in INPUTS])
def test_inputs_leave_the_margin_rule_nearly_every_pixel(make, K, H, W, without):
    logits = make()
    if without is not None:
        a, b = UR.TWIN
        assert b == without and torch.equal(logits[..., a], logits[..., b])
    share = _undecided(logits, K, H, W, without)
    print(f"below the margin: {100 * share:.4f} %")
    assert share <= UR.MAX_UNDECIDED, share


def test_inputs_that_were_left_out_would_not_qualify():
    """Why two branches have one field only. W = 1 (130 output pixels): a single near-tie of
    the noise field is 0.8 % of the map. Downsampling 33 -> 17: every output pixel is a source
    pixel, and bf16 noise ties its top two classes exactly at about 1 % of them."""
    for B, h, w, H, W, K, ldk in [(2, 9, 3, 65, 1, 21, 24), (2, 33, 33, 17, 17, 21, 24)]:
        fields = [s[8] for s in UR.UPSAMPLE_SHAPES if s[:7] == (B, h, w, H, W, K, ldk)]
        assert len(fields) == 1 and "noise" not in fields[0]
        assert _undecided(UR.make_logits(B, h, w, K, ldk, "noise"), K, H, W, None) > UR.MAX_UNDECIDED
