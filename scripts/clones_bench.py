"""ms per training step of the joint fp32 model with num_clones = K clones of b rows each, (K, b) = (1, 256), (2, 128), (4, 64),
(8, 32), against K times the plain step at b rows on the same build: the difference is what running the clones back to back
costs on top of their own steps (K accumulation launches, K - 1 fewer Adam launches, the re-launch gaps).  ONE process, one
net, device events around each window, every shape warmed up before it is timed, min / median / max of the windows.

    python scripts/clones_bench.py [--windows 5] [--iters-scale 1.0] [--out profiles/clones.json]

A step of K clones of b rows and a step of K b rows compute different things (per-clone BatchNorm statistics), so the first
row of each pair is a cost report, not a race.  Needs the GPU (no fallback).  bench.py (the flagship benchmark) is a different
measurement and is not touched."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tumblr_emotions_amd import _lib                          # noqa: E402
from tumblr_emotions_amd.net import SentimentNet              # noqa: E402
from tumblr_emotions_amd.synthetic import synthetic_batch_numpy, to_device      # noqa: E402

TOTAL = 256
CLONES = (1, 2, 4, 8)


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


def measure(net, batch, K, windows, iters):
    kw = {"num_clones": K} if K > 1 else {}

    def step():
        net.train_step(batch, 1e-4, **kw)
    window_ms(step, 3)                                        # this shape's buffers, plans and clocks
    ms = [window_ms(step, iters) for _ in range(windows)]
    assert bool(torch.isfinite(net.store.theta).all())
    return spread(ms)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--iters-scale", type=float, default=1.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clones.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "clones_bench.py needs the GPU"
    _lib.load()
    net = SentimentNet(mode="joint", nb_emotions=15, vocab_size=1000, embedding_dim=50, post_size=50)
    net.initialize(seed=1)
    whole = to_device(synthetic_batch_numpy(TOTAL, 50, 1000, seed=2))
    rows = []
    for K in CLONES:
        b = TOTAL // K
        iters = max(3, int(args.iters_scale * 8))
        clones = measure(net, whole, K, args.windows, iters)
        # the plain step at b rows: the first b rows of the same batch (the engines re-allocate at every change of shape)
        single = clones if K == 1 else measure(net, {k: v[:b] for k, v in whole.items()}, 1, args.windows, iters * min(K, 4))
        row = {"num_clones": K, "clone_batch": b, "rows_per_step": TOTAL, "step_ms": clones, "single_clone_step_ms": single,
               "k_times_single_ms": K * single["median"], "difference_ms": clones["median"] - K * single["median"],
               "samples_per_s": TOTAL / (clones["median"] * 1e-3)}
        rows.append(row)
        print("K=%d x %-3d  step %.3f ms [%.3f, %.3f]   plain step at %d rows %.3f ms   K x plain %.3f ms   difference %+.3f ms" % (
            K, b, clones["median"], clones["min"], clones["max"], b, single["median"], row["k_times_single_ms"],
            row["difference_ms"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "model": "joint fp32, rnn_size 512, post_size 50", "rows": rows}, f,
                  indent=1)
    print("wrote", args.out)
