"""What moving averages of the trained weights cost on the joint fp32 training step, at B = 256 and B = 32:

  * key absent against moving_average_decay set (ds_adam_tf_ema replaces ds_adam_tf: no extra launch, one more stream read
    and one more written, 8 * n_trainable_padded bytes per step) -- two nets in ONE process, timed as interleaved windows
    (the method and the helpers of scripts/grad_clip_bench.py), median / min / max of the windows;
  * with --parent-tree DIR: key absent against the package of another checkout (the parent commit, built in DIR), loaded into
    the same process under another module name -- the step without the key must be the parent's step;
  * one averaged_weights() round trip (enter and exit: two exchanges of theta and store.ema, nothing run inside), at B = 256
    only -- what validation during training pays on top of its batches.

    python scripts/ema_bench.py [--windows 5] [--iters 20] [--parent-tree DIR] [--out profiles/ema.json]

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

DECAY = 0.9999


def round_trip(net):
    with net.averaged_weights():
        pass


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ema.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "ema_bench.py needs the GPU"
    _lib.load()
    ParentNet = None
    if args.parent_tree:
        ParentNet, parent_lib = load_package(os.path.abspath(args.parent_tree), "tumblr_emotions_amd_parent")
        parent_lib.load()
        assert os.path.realpath(parent_lib.LIB_PATH) != os.path.realpath(_lib.LIB_PATH)
    rows = []
    for B in BATCHES:
        batch = to_device(synthetic_batch_numpy(B, 50, 1000, seed=2))
        nets = {"absent": SentimentNet(**DIMS), "moving_average_decay": SentimentNet(moving_average_decay=DECAY, **DIMS)}
        if ParentNet is not None:
            nets["parent"] = ParentNet(**DIMS)
        for net in nets.values():
            net.initialize(seed=1)
        iters = args.iters if B >= 128 else 3 * args.iters
        res = interleaved({k: stepper(n, batch) for k, n in nets.items()}, args.windows, iters)
        for k, n in nets.items():
            assert bool(torch.isfinite(n.store.theta).all()), k
        on, off = nets["moving_average_decay"], nets["absent"]
        assert off.store.ema is None and bool(torch.isfinite(on.store.ema).all())
        st = off.store
        row = {"batch": B, "iters_per_window": iters, "step_ms": res,
               "ema_minus_absent_ms": res["moving_average_decay"]["median"] - res["absent"]["median"],
               "trainable_elements": int(st.n_trainable), "trainable_padded": int(st.n_trainable_padded),
               "added_bytes_per_step": 8 * int(st.n_trainable_padded),
               "ema_equals_absent_bit_for_bit": bool(all(torch.equal(getattr(on.store, x), getattr(off.store, x))
                                                         for x in ("theta", "m", "v")))}
        if ParentNet is not None:
            p, o = res["parent"], res["absent"]
            row["absent_minus_parent_ms"] = o["median"] - p["median"]
            row["absent_inside_parent_spread"] = bool(p["min"] <= o["median"] <= p["max"])
            row["absent_equals_parent_bit_for_bit"] = bool(all(
                torch.equal(getattr(off.store, x), getattr(nets["parent"].store, x)) for x in ("theta", "m", "v")))
        if B == BATCHES[0]:
            window_ms(lambda: round_trip(on), 3)
            row["averaged_weights_round_trip_ms"] = spread([window_ms(lambda: round_trip(on), 20) for _ in range(args.windows)])
        rows.append(row)
        print(json.dumps(row), flush=True)
        del nets, on, off
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "model": "joint fp32, rnn_size 512, post_size 50, synthetic batch",
                   "moving_average_decay": DECAY,
                   "method": "interleaved windows in one process, device events, %d windows" % args.windows, "rows": rows},
                  f, indent=1)
    print("wrote", args.out)
