"""Forward-only images/s of SentimentNet.predict(is_training=False), unfused against fused (BatchNorm + ReLU in the conv
epilogue), in ONE process with alternating windows: device events around each window, every shape warmed up first, the
spread of the windows reported next to their median.  Batches 1, 32, 256; modes image and joint; a synthetic batch.
Also a per-layer microbenchmark at one batch: each fusable conv plan, conv -> ds_bn_apply_relu against the fused launch.

    python scripts/inference_bench.py [--windows 7] [--iters-scale 1.0] [--layer-batch 256] [--out profiles/inference.json]

Needs the GPU (no fallback).  bench.py (the training-step benchmark) is a different measurement and is not touched."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tumblr_emotions_amd import _lib, ops                     # noqa: E402
from tumblr_emotions_amd.net import SentimentNet              # noqa: E402
from tumblr_emotions_amd.synthetic import synthetic_batch_numpy, to_device      # noqa: E402


def window_ms(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def spread(xs):
    xs = sorted(xs)
    return {"median": float(np.median(xs)), "min": xs[0], "max": xs[-1]}


def model_bench(mode, B, windows, scale):
    kw = dict(nb_emotions=15) if mode == "image" else dict(nb_emotions=15, vocab_size=1000, embedding_dim=50, post_size=50)
    net = SentimentNet(mode=mode, **kw)
    net.initialize(seed=1)
    V = 10 if mode == "image" else 1000
    T = 8 if mode == "image" else 50
    tr = to_device(synthetic_batch_numpy(8, T, V, seed=1))
    for _ in range(2):                                        # moving statistics off their initial values
        net.train_step(tr, 1e-3)
    batch = to_device(synthetic_batch_numpy(B, T, V, seed=2))
    a = net.predict(batch, fused=False).clone()
    b = net.predict(batch, fused=True).clone()
    same = bool(torch.equal(a, b))
    iters = max(3, int(scale * {1: 60, 32: 30, 256: 8}.get(B, 8)))
    runs = {"unfused": lambda: net.predict(batch, fused=False), "fused": lambda: net.predict(batch, fused=True)}
    for name in ("unfused", "fused", "unfused", "fused"):    # warm-up, both orders of the transition
        window_ms(runs[name], 3)
    ms = {"unfused": [], "fused": []}
    for _ in range(windows):                                  # alternating windows in one process
        for name in ("unfused", "fused"):
            window_ms(runs[name], 1)                          # (the first call after a switch prepares the statistics again)
            ms[name].append(window_ms(runs[name], iters))
    out = {"mode": mode, "batch": B, "iters_per_window": iters, "windows": windows, "bit_identical": same,
           "fallback_layers": [list(r) for r in net.fused_report()]}
    for name in ms:
        s = spread(ms[name])
        out[name] = {"ms_per_call": s, "images_per_s": {"median": B / s["median"] * 1e3, "min": B / s["max"] * 1e3,
                                                        "max": B / s["min"] * 1e3}}
    out["speedup_median"] = out["unfused"]["ms_per_call"]["median"] / out["fused"]["ms_per_call"]["median"]
    del net
    torch.cuda.empty_cache()
    return out


def layer_bench(B, windows):
    """Every fusable forward plan of the tower on its own, on private copies of the plans: conv + ds_bn_apply_relu against
    the fused launch (us per layer, median and spread of windows of at least 0.1 s each)."""
    net = SentimentNet(mode="image", nb_emotions=15)
    net.initialize(seed=1)
    net.predict(to_device(synthetic_batch_numpy(B, 8, 10, seed=3)), fused=True)
    rows = []
    for l in net.image.layers:
        if l.fold:
            continue
        plain_plan = l.fwd.copy()
        d = plain_plan.d
        d.ldx, d.ldz, d.flags, d.norm_rstd, d.norm_shift = l.cin, l.cout, 0, None, None
        q = plain_plan.bn_relu_variant(l.cout)
        if q is None:
            continue
        x = torch.rand(B, l.H, l.W, l.cin, device="cuda") * 2 - 1
        y = torch.empty(l.M, l.cout, device="cuda")
        z = torch.empty(l.M, l.cout, device="cuda")
        segs = ops.make_segments([(0, l.cout, y.data_ptr(), l.cout)])
        sc, sh = torch.rand(l.cout, device="cuda") + 0.5, torch.rand(l.cout, device="cuda") - 0.5

        def plain():
            plain_plan.run(ops._p(x), l.w_ptr, ops._p(z))
            ops.bn_apply_relu(z, l.M, l.cout, sc, sh, segs)

        def fused():
            q.run_bn_relu(ops._p(x), l.w_ptr, ops._p(y), sc.data_ptr(), sh.data_ptr())
        iters = {}
        for name, f in (("plain", plain), ("fused", fused)):
            window_ms(f, 3)
            iters[name] = max(10, int(100.0 / max(window_ms(f, 5), 1e-3)) + 1)      # windows of about 0.1 s
        t = {"plain": [], "fused": []}
        for _ in range(windows):
            t["plain"].append(window_ms(plain, iters["plain"]) * 1e3)
            t["fused"].append(window_ms(fused, iters["fused"]) * 1e3)
        rows.append({"layer": l.key.replace("InceptionV1/", ""), "family": int(q.family), "splitk": int(q.splitk),
                     "k": l.k, "launches_per_window": iters, "plain_us": spread(t["plain"]), "fused_us": spread(t["fused"])})
    del net
    torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--iters-scale", type=float, default=1.0)
    ap.add_argument("--batches", type=int, nargs="*", default=[1, 32, 256])
    ap.add_argument("--modes", nargs="*", default=["image", "joint"])
    ap.add_argument("--layer-batch", type=int, default=256, help="0: skip the per-layer microbenchmark")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "inference.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("inference_bench.py measures on the GPU; none found (no fallback)")
    _lib.load()
    res = {"device": torch.cuda.get_device_name(0), "timing": "device events around windows of predict() calls, "
           "alternating unfused / fused in one process; spread = min / median / max over the windows", "models": [], "layers": []}
    for mode in a.modes:
        for B in a.batches:
            r = model_bench(mode, B, a.windows, a.iters_scale)
            print(json.dumps({k: r[k] for k in ("mode", "batch", "bit_identical", "speedup_median")} |
                             {"unfused_ms": r["unfused"]["ms_per_call"], "fused_ms": r["fused"]["ms_per_call"]}), flush=True)
            res["models"].append(r)
    if a.layer_batch:
        res["layer_batch"] = a.layer_batch
        res["layers"] = layer_bench(a.layer_batch, max(3, a.windows // 2))
        for r in res["layers"]:
            print("%-44s fam %d  plain %8.1f us  fused %8.1f us" % (r["layer"], r["family"], r["plain_us"]["median"],
                                                                    r["fused_us"]["median"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
