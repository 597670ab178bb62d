#!/usr/bin/env python
"""Branch_3 of Mixed_3b .. 5b at batch B (default 256): MaxPool 3x3 / 1 -> Conv2d_0b_1x1 as ONE launch of the wide kernel
(ds_conv_desc.pool_argmax) against the pool pass followed by the plain conv.  Three input buffers in rotation, so a launch
does not find its input in the caches.  Prints one line per layer and the sums; `python scripts/pool_on_load_bench.py 256 json`
adds one JSON line."""
import json
import os
import sys

sys.path.insert(0, os.environ.get("DS_TREE") or os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from tumblr_emotions_amd import ops

B = int(sys.argv[1]) if len(sys.argv) > 1 else 256
# (block, HW, Cin, Cout, input is raw z normalised on load)
LAYERS = [("3b", 28, 192, 32, False), ("3c", 28, 256, 64, True), ("4b", 14, 480, 64, False), ("4c", 14, 512, 64, True),
          ("4d", 14, 512, 64, True), ("4e", 14, 512, 64, True), ("4f", 14, 528, 128, True), ("5b", 7, 832, 128, False)]


def timeit(f, reps=12):
    for i in range(3):
        f(i)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(reps):
        f(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


tot = [0.0, 0.0]
rows = []
print("%3s %3s %4s %4s | %9s %7s | %9s | %5s" % ("", "HW", "K", "N", "fused us", "TB/s", "2-pass us", "ratio"))
for name, hw, K, N, norm in LAYERS:
    M = B * hw * hw
    xs = [torch.randn(B, hw, hw, K, device="cuda") for _ in range(3)]
    w = torch.randn(K, N, device="cuda") * 0.05
    r, sh = torch.rand(K, device="cuda") + 0.5, torch.randn(K, device="cuda") * 0.3
    z = torch.empty(M, N, device="cuda")
    am = torch.empty(M, K, dtype=torch.uint8, device="cuda")
    pooled = torch.empty(B, hw, hw, K, device="cuda")
    fused = ops.LayerPlan(ops.DS_CONV_FWD, ops.DS_ARITH_F32, 0, B, hw, hw, K, N, 1, 1, K, N, ops.DS_EPI_STATS)
    assert fused.enable_pool3(am)
    if norm:
        fused.d.norm_rstd, fused.d.norm_shift = r.data_ptr(), sh.data_ptr()
    plain = ops.LayerPlan(ops.DS_CONV_FWD, ops.DS_ARITH_F32, 0, B, hw, hw, K, N, 1, 1, K, N, ops.DS_EPI_STATS)
    stats = torch.zeros(2 * N * max(fused.partials, plain.partials), device="cuda")

    def two_pass(i):
        if norm:
            ops.maxpool_bn_relu_fwd(xs[i % 3], r, sh, pooled, am, B, hw, hw, K, 3, 1)
        else:
            ops.maxpool_fwd(xs[i % 3], pooled, am, B, hw, hw, K, 3, 1, "SAME")
        plain.run(ops._p(pooled), ops._p(w), ops._p(z), stats=ops._p(stats))

    tf = timeit(lambda i: fused.run(ops._p(xs[i % 3]), ops._p(w), ops._p(z), stats=ops._p(stats)))
    t2 = timeit(two_pass)
    nbytes = M * (4 * K + K + 4 * N)          # x read once, winners and z written
    tot[0] += tf
    tot[1] += t2
    rows.append(dict(block=name, hw=hw, K=K, N=N, fused_us=round(tf, 2), two_pass_us=round(t2, 2), bytes=nbytes))
    print("%3s %3d %4d %4d | %9.1f %7.2f | %9.1f | %5.2f" % (name, hw, K, N, tf, nbytes / tf / 1e6, t2, t2 / tf))
nb = sum(r["bytes"] for r in rows)
print("sum: fused %.1f us (%.2f TB/s over %.0f MB), two passes %.1f us" % (tot[0], nb / tot[0] / 1e6, nb / 1e6, tot[1]))
if len(sys.argv) > 2:
    print(json.dumps(dict(batch=B, fused_us=round(tot[0], 1), two_pass_us=round(tot[1], 1), layers=rows)))
