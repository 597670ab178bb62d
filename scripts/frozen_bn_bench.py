"""ms per training step of the normal step (batch statistics) against the frozen-BatchNorm step (SentimentNet(frozen_bn=True):
moving statistics inside the train step), in ONE process with alternating windows: device events around each window, every
shape warmed up first, the spread of the windows reported next to their median.  Batches 256 and 32; modes joint and image; a
synthetic batch.  Also the library calls per step of either (counted through _lib.check: one per entry-point call).

    python scripts/frozen_bn_bench.py [--windows 7] [--iters-scale 1.0] [--out profiles/frozen_bn.json]

The two steps compute different things, so this is a cost report, not a race.  Needs the GPU (no fallback).  bench.py (the
flagship benchmark) is a different measurement and is not touched."""
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


def calls_per_step(fn):
    """Library entry-point calls of one step, by name."""
    seen = {}
    real = _lib.check

    def counting(rc, what):
        seen[what] = seen.get(what, 0) + 1
        return real(rc, what)
    _lib.check = counting
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        _lib.check = real
    return seen


def model_bench(mode, B, windows, scale):
    kw = dict(nb_emotions=15) if mode == "image" else dict(nb_emotions=15, vocab_size=1000, embedding_dim=50, post_size=50)
    V, T = (10, 8) if mode == "image" else (1000, 50)
    batch = to_device(synthetic_batch_numpy(B, T, V, seed=2))
    nets = {}
    for name in ("normal", "frozen"):
        net = SentimentNet(mode=mode, frozen_bn=(name == "frozen"), **kw)
        net.initialize(seed=1)
        nets[name] = net
    for _ in range(2):                                        # moving statistics off their initial values, shared by both nets
        nets["normal"].train_step(batch, 1e-3)
    torch.cuda.synchronize()
    nets["frozen"].store.frozen.copy_(nets["normal"].store.frozen)
    nets["frozen"].after_load()
    runs = {name: (lambda n=net: n.train_step(batch, 1e-4)) for name, net in nets.items()}
    iters = max(3, int(scale * {32: 30, 256: 8}.get(B, 8)))
    for name in ("normal", "frozen", "normal", "frozen"):
        window_ms(runs[name], 3)
    ms = {"normal": [], "frozen": []}
    for _ in range(windows):
        for name in ("normal", "frozen"):
            ms[name].append(window_ms(runs[name], iters))
    out = {"mode": mode, "batch": B, "iters_per_window": iters, "windows": windows}
    for name in ms:
        calls = calls_per_step(runs[name])
        bn = {k: v for k, v in calls.items() if k.startswith("ds_bn_")}
        out[name] = {"ms_per_step": spread(ms[name]), "library_calls": sum(calls.values()), "bn_calls": bn,
                     "finite": bool(torch.isfinite(nets[name].store.theta).all())}
    out["frozen_over_normal_median"] = out["frozen"]["ms_per_step"]["median"] / out["normal"]["ms_per_step"]["median"]
    del nets, runs
    torch.cuda.empty_cache()
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--iters-scale", type=float, default=1.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frozen_bn.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "frozen_bn_bench.py needs the GPU"
    _lib.load()
    rows = []
    for mode in ("joint", "image"):
        for B in (256, 32):
            r = model_bench(mode, B, args.windows, args.iters_scale)
            rows.append(r)
            print("%-5s B=%-3d normal %.3f ms [%.3f, %.3f]  frozen %.3f ms [%.3f, %.3f]  ratio %.3f  calls %d -> %d" % (
                mode, B, r["normal"]["ms_per_step"]["median"], r["normal"]["ms_per_step"]["min"], r["normal"]["ms_per_step"]["max"],
                r["frozen"]["ms_per_step"]["median"], r["frozen"]["ms_per_step"]["min"], r["frozen"]["ms_per_step"]["max"],
                r["frozen_over_normal_median"], r["normal"]["library_calls"], r["frozen"]["library_calls"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "rows": rows}, f, indent=1)
    print("wrote", args.out)
