"""What label_smoothing and class_weights cost on the joint fp32 training step, at B = 256 and B = 32:

  * two arms -- the keys absent (the ds_slab_epilogue_ce launch, as before) and both keys set (ds_slab_epilogue_ce_opts: one
    more pass over the B labels in the same single workgroup) -- nets in ONE process, timed as interleaved windows (the method
    and the helpers of scripts/grad_clip_bench.py, as scripts/ema_bench.py), median / min / max of the windows;
  * with --parent-tree DIR: a third arm, the package of another checkout (the parent commit, built in DIR), loaded into the
    same process under another module name -- the step without the keys must be the parent's step, bit for bit, and its
    median must lie inside the spread of the parent's own windows;
  * the two cross-entropy launches alone, old form and new form: ds_softmax_ce / ds_softmax_ce_opts on B x 15 logits and
    ds_slab_epilogue_ce / ds_slab_epilogue_ce_opts on eight slabs of them.

    python scripts/loss_options_bench.py [--windows 5] [--iters 20] [--parent-tree DIR] [--out profiles/loss_options.json]

Needs the GPU (no fallback).  bench.py (the flagship benchmark) is a different measurement and is not touched."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from grad_clip_bench import BATCHES, DIMS, interleaved, load_package, spread, stepper, window_ms      # noqa: E402
from tumblr_emotions_amd import _lib, ops                     # noqa: E402
from tumblr_emotions_amd.net import SentimentNet              # noqa: E402
from tumblr_emotions_amd.synthetic import synthetic_batch_numpy, to_device      # noqa: E402

NC = 15
WEIGHTS = [0.5 + 0.1 * c for c in range(NC - 1)] + [0.0]
ARMS = {"absent": {}, "both_keys": {"label_smoothing": 0.1, "class_weights": WEIGHTS}}


def launches_alone(B, windows):
    """The four launches on their own buffers, back to back out of the cache: the kernel's own time."""
    lib = _lib.load()
    g = torch.Generator(device="cuda").manual_seed(B)
    logits = torch.randn(B, NC, device="cuda", generator=g)
    slabs = torch.randn(8, B, NC, device="cuda", generator=g)
    bias = torch.randn(NC, device="cuda", generator=g)
    labels = torch.randint(0, NC, (B,), device="cuda", generator=g)
    cw = torch.tensor(WEIGHTS, device="cuda")
    ce = ops.ce_desc(0.1, cw)
    loss, dl, out = torch.zeros(1, device="cuda"), torch.empty(B, NC, device="cuda"), torch.empty(B, NC, device="cuda")
    fns = {"ds_softmax_ce": lambda: ops.softmax_ce(logits, labels, B, NC, 1.0, None, loss, dl),
           "ds_softmax_ce_opts": lambda: ops.softmax_ce_opts(ce, logits, labels, B, NC, 1.0, None, loss, dl)}
    if B <= 512:
        import ctypes as C
        s = ops._p(slabs)
        fns["ds_slab_epilogue_ce"] = lambda: _lib.check(lib.ds_slab_epilogue_ce(
            s, 8, B * NC, NC, B, NC, ops._p(out), ops._p(bias), ops._p(labels), 1.0, None, ops._p(loss), ops._p(dl),
            ops._stream()), "ds_slab_epilogue_ce")
        fns["ds_slab_epilogue_ce_opts"] = lambda: _lib.check(lib.ds_slab_epilogue_ce_opts(
            C.byref(ce), s, 8, B * NC, NC, B, NC, ops._p(out), ops._p(bias), ops._p(labels), 1.0, None, ops._p(loss),
            ops._p(dl), ops._stream()), "ds_slab_epilogue_ce_opts")
    res = {}
    for k, fn in fns.items():
        window_ms(fn, 5)
    for k, fn in fns.items():
        res[k] = spread([window_ms(fn, 200) for _ in range(windows)])
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loss_options.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "loss_options_bench.py needs the GPU"
    _lib.load()
    ParentNet = None
    if args.parent_tree:
        ParentNet, parent_lib = load_package(os.path.abspath(args.parent_tree), "tumblr_emotions_amd_parent")
        parent_lib.load()
        assert os.path.realpath(parent_lib.LIB_PATH) != os.path.realpath(_lib.LIB_PATH)
    rows = []
    for B in BATCHES:
        batch = to_device(synthetic_batch_numpy(B, 50, 1000, seed=2))
        nets = {k: SentimentNet(**dict(DIMS, **kw)) for k, kw in ARMS.items()}
        if ParentNet is not None:
            nets["parent"] = ParentNet(**DIMS)
        for net in nets.values():
            net.initialize(seed=1)
        iters = args.iters if B >= 128 else 3 * args.iters
        res = interleaved({k: stepper(n, batch) for k, n in nets.items()}, args.windows, iters)
        for k, n in nets.items():
            assert bool(torch.isfinite(n.store.theta).all()), k
        off = nets["absent"]

        def same(a, b):
            return bool(all(torch.equal(getattr(a.store, x), getattr(b.store, x)) for x in ("theta", "m", "v")))

        row = {"batch": B, "iters_per_window": iters, "step_ms": res,
               "both_keys_minus_absent_ms": res["both_keys"]["median"] - res["absent"]["median"],
               "both_keys_differs_from_absent": not same(nets["both_keys"], off)}
        if ParentNet is not None:
            p, o = res["parent"], res["absent"]
            row["parent_spread_ms"] = p["max"] - p["min"]
            row["absent_inside_parent_spread"] = bool(p["min"] <= o["median"] <= p["max"])
            row["absent_equals_parent_bit_for_bit"] = same(off, nets["parent"])
        row["ce_launch_ms"] = launches_alone(B, args.windows)
        rows.append(row)
        print(json.dumps(row), flush=True)
        del nets, off
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "model": "joint fp32, rnn_size 512, post_size 50, synthetic batch",
                   "arms": ARMS, "method": "interleaved windows in one process, device events, %d windows" % args.windows,
                   "rows": rows}, f, indent=1)
    print("wrote", args.out)
