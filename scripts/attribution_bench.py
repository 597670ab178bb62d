"""ms per call of SentimentNet.eval_gradients (moving-statistics gradients: pointwise BatchNorm backward) against
SentimentNet.input_gradient (batch-statistics gradients: reduce + finalize + apply per layer) on the same joint net, in ONE
process with alternating windows: device events around each window, both warmed up first, the spread of the windows reported
next to their median.  Batches 1, 8, 32.  Also the number of kernel-library calls each makes (every ops wrapper reports
through _lib.check once per call; a call is one launch, a few for split-K plans).

    python scripts/attribution_bench.py [--windows 7] [--iters-scale 1.0] [--out profiles/attribution.json]

The two compute DIFFERENT gradients (eval_gradients also differentiates the text tower); the comparison says what the
moving-statistics backward chain costs next to the batch-statistics one.  Needs the GPU (no fallback)."""
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


def library_calls(fn):
    """Kernel-library calls of one fn(), by name."""
    seen = {}
    real = _lib.check

    def check(rc, what):
        seen[what] = seen.get(what, 0) + 1
        return real(rc, what)
    _lib.check = check
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        _lib.check = real
    return seen


def bench(B, windows, scale):
    V, T = 1000, 50
    net = SentimentNet(mode="joint", nb_emotions=15, vocab_size=V, embedding_dim=50, post_size=T)
    net.initialize(seed=1)
    tr = to_device(synthetic_batch_numpy(8, T, V, seed=1))
    for _ in range(2):                                        # moving statistics off their initial values
        net.train_step(tr, 1e-3)
    batch = to_device(synthetic_batch_numpy(B, T, V, seed=2))
    batch = {k: batch[k] for k in ("images", "texts", "seq_lens")}
    ones = torch.ones(B, 1024, device="cuda")
    runs = {"eval_gradients": lambda: net.eval_gradients(batch, 3),
            "input_gradient": lambda: net.input_gradient(batch, 3, dropout_mask=ones)}
    for name in ("input_gradient", "eval_gradients", "input_gradient", "eval_gradients"):          # warm-up, both transitions
        window_ms(runs[name], 3)
    calls = {name: library_calls(runs[name]) for name in runs}
    # windows of about half a second each (a window of a few hundredths of a second mostly times the clock and the scheduler)
    iters = max(3, int(scale * 500.0 / max(window_ms(runs["input_gradient"], 5), 1e-3)) + 1)
    ms = {name: [] for name in runs}
    for _ in range(windows):                                  # alternating windows in one process
        for name in runs:
            window_ms(runs[name], 1)
            ms[name].append(window_ms(runs[name], iters))
    out = {"mode": "joint", "batch": B, "iters_per_window": iters, "windows": windows}
    for name in runs:
        out[name] = {"ms_per_call": spread(ms[name]), "library_calls": int(sum(calls[name].values())),
                     "calls_by_name": dict(sorted(calls[name].items()))}
    out["ratio_median"] = out["input_gradient"]["ms_per_call"]["median"] / out["eval_gradients"]["ms_per_call"]["median"]
    del net
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--iters-scale", type=float, default=1.0)
    ap.add_argument("--batches", type=int, nargs="*", default=[1, 8, 32])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attribution.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("attribution_bench.py measures on the GPU; none found (no fallback)")
    _lib.load()
    res = {"device": torch.cuda.get_device_name(0), "timing": "device events around windows of calls, alternating "
           "eval_gradients / input_gradient in one process; spread = min / median / max over the windows", "runs": []}
    for B in a.batches:
        r = bench(B, a.windows, a.iters_scale)
        print(json.dumps({"batch": B, "ratio_median": r["ratio_median"],
                          "eval_gradients_ms": r["eval_gradients"]["ms_per_call"], "eval_gradients_calls": r["eval_gradients"]["library_calls"],
                          "input_gradient_ms": r["input_gradient"]["ms_per_call"], "input_gradient_calls": r["input_gradient"]["library_calls"]}),
              flush=True)
        res["runs"].append(r)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
