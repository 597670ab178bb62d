"""What the choice of optimiser costs on the joint fp32 training step, at B = 256 and B = 32:

  * five arms -- `optimizer` absent, 'adam' given explicitly (both the ds_adam_tf launch), 'sgd', 'momentum', 'rmsprop' (one
    ds_opt_step each: 12 / 20 / 28 bytes per element against Adam's 28) -- nets in ONE process, timed as interleaved windows
    (the method and the helpers of scripts/grad_clip_bench.py), median / min / max of the windows;
  * with --parent-tree DIR: a sixth arm, the package of another checkout (the parent commit, built in DIR), loaded into the
    same process under another module name -- the step without the key must be the parent's step, bit for bit;
  * the optimiser launch alone (net._optimise on the step's own buffers), per arm: the kernel's own time.

    python scripts/optimizers_bench.py [--windows 5] [--iters 20] [--parent-tree DIR] [--out profiles/optimizers.json]

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
from tumblr_emotions_amd import _lib                          # noqa: E402
from tumblr_emotions_amd.net import SentimentNet              # noqa: E402
from tumblr_emotions_amd.synthetic import synthetic_batch_numpy, to_device      # noqa: E402

ARMS = {"absent": {}, "adam": {"optimizer": "adam"}, "sgd": {"optimizer": "sgd"}, "momentum": {"optimizer": "momentum"},
        "rmsprop": {"optimizer": "rmsprop"}}
BYTES_PER_ELEMENT = {"absent": 28, "adam": 28, "sgd": 12, "momentum": 20, "rmsprop": 28, "parent": 28}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optimizers.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "optimizers_bench.py needs the GPU"
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
        st = off.store

        def same(a, b):
            return bool(all(torch.equal(getattr(a.store, x), getattr(b.store, x)) for x in ("theta", "m", "v")))

        row = {"batch": B, "iters_per_window": iters, "step_ms": res,
               "trainable_elements": int(st.n_trainable), "trainable_padded": int(st.n_trainable_padded),
               "minus_absent_ms": {k: res[k]["median"] - res["absent"]["median"] for k in res if k != "absent"},
               "adam_equals_absent_bit_for_bit": same(nets["adam"], off)}
        if ParentNet is not None:
            p, o = res["parent"], res["absent"]
            row["parent_spread_ms"] = p["max"] - p["min"]
            row["absent_inside_parent_spread"] = bool(p["min"] <= o["median"] <= p["max"])
            row["absent_equals_parent_bit_for_bit"] = same(off, nets["parent"])
            row["slower_than_adam_by_more_than_parent_spread"] = [
                k for k in ("sgd", "momentum", "rmsprop") if res[k]["median"] - res["adam"]["median"] > p["max"] - p["min"]]
        # the optimiser launch alone, on the buffers the steps left (lr 0; the slots still move)
        alone = {}
        for k, n in nets.items():
            fn = (lambda n=n: n._optimise(1.0, 0.0))
            window_ms(fn, 5)
            alone[k] = spread([window_ms(fn, 50) for _ in range(args.windows)])
            alone[k]["stream_bytes"] = BYTES_PER_ELEMENT[k] * int(st.n_trainable_padded)
        row["optimiser_launch_ms"] = alone
        rows.append(row)
        print(json.dumps(row), flush=True)
        del nets, off
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "model": "joint fp32, rnn_size 512, post_size 50, synthetic batch",
                   "arms": {k: v for k, v in ARMS.items()},
                   "method": "interleaved windows in one process, device events, %d windows" % args.windows, "rows": rows},
                  f, indent=1)
    print("wrote", args.out)
