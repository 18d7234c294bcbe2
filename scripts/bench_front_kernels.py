"""Standalone timing of the front kernels at the B = 32 headline shapes (513^2, 640x480
camera, the committed picks' band heights): back-to-back launches of one kernel, every row
computed ("off") and with the letterbox's constant rows computed once ("on", ops/row_repeat.py),
checked equal. Run from the root of the tree to be timed; a tree without ops/row_repeat.py
gives the "off" lines only, so two checkouts can be compared:

  python scripts/bench_front_kernels.py
"""
import os, sys, json
sys.path.insert(0, os.getcwd()); sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
import numpy as np, torch
from semantic_segmentation_server_amd.ops import hip_ops as K, fused_band as FB, reference_ops as R_
from test_fused_band_cpu import band_block, pack_band
try:
    from semantic_segmentation_server_amd.ops import row_repeat as RR
except ImportError:
    RR = None
DEV, B, H = "cuda", 32, 513
K._hip_mod()
lx, ly, *_ = R_.letterbox_luts(640, 480, H, H)
lxd = torch.tensor(np.array(lx), dtype=torch.int32, device=DEV)
lyd = torch.tensor(np.array(ly), dtype=torch.int32, device=DEV)

def timeit(fn, n=40, reps=5):
    for _ in range(5): fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n): fn()
        b.record(); torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) * 1e3 / n)
    return min(ts), sorted(ts)[len(ts) // 2]

res = {}
# stem
from semantic_segmentation_server_amd.models.layers import ConvBNAct, init_random
from semantic_segmentation_server_amd.models.mobilenetv2 import InvertedResidual, IRSpec
stem = ConvBNAct(3, 32, 3, 2, act="relu6"); blk = InvertedResidual(IRSpec(32, 16, 1, 1, 1))
init_random(stem, seed=5); init_random(blk, seed=6); stem.eval(); blk.eval()
dwf, dbf = blk.dw.fold(); pwf, pbf = blk.project.fold()
P = K.pack_stem_block0(stem, dwf[:, 0], dbf, pwf[:, :, 0, 0], pbf, DEV)
fd = torch.randint(0, 256, (B, 480, 640, 3), dtype=torch.uint8).to(DEV)
out = torch.zeros((B, 257, 257, 16), dtype=torch.bfloat16, device=DEV)
res["stem off"] = timeit(lambda: K.stem_band(fd, lxd, lyd, P, out, H=H, W=H, R=29, nbx=5, one_barrier=True))
if RR:
    ref = out.clone()
    res["stem on"] = timeit(lambda: K.stem_band(fd, lxd, lyd, P, out, H=H, W=H, R=29, nbx=5, one_barrier=True, row_repeat=True))
    assert torch.equal(ref, out)
rf = (2, 3, 3)
x = out
for name, cin, cout, s, IH, R, nw in [("block1", 16, 24, 2, 257, 33, 5), ("block2", 24, 24, 1, 129, 17, 3),
                                      ("block3", 24, 32, 2, 129, 17, 3), ("block4", 32, 32, 1, 65, 9, 2),
                                      ("block5", 32, 32, 1, 65, 9, 2), ("block6", 32, 64, 2, 65, 7, 1)]:
    b_, spec = band_block(cin, cout, s, seed=cin + cout)
    pk = pack_band(b_, spec, device=DEV)
    OH = (IH - 1) // s + 1
    o = torch.zeros((B, OH, OH, cout), dtype=torch.bfloat16, device=DEV)
    kw = dict(B=B, IH=IH, IW=IH, stride=s, residual=spec.residual, R=R, nw=nw, one_barrier=True)
    if RR: rf = RR.rf_conv3x3(rf, s)
    if name in ("block4", "block5"):
        FB.fused_ir_slice(x, pk, o, **kw); x = o; continue
    res[name + " off"] = timeit(lambda: FB.fused_ir_slice(x, pk, o, **kw))
    if RR:
        ref = o.clone()
        res[name + " on"] = timeit(lambda: FB.fused_ir_slice(x, pk, o, lut_y=lyd, H=H, rf=rf, **kw))
        assert torch.equal(ref, o), name
        print(name, rf, RR.zone(RR.pad_start(ly), H, OH, rf))
    x = o
for k, v in res.items(): print(f"{k:12s} min {v[0]:7.1f} us  median {v[1]:7.1f} us")
