"""What gradient clipping costs on the joint fp32 training step, at B = 256 and B = 32:

  * keys off against clip_global_norm on (two more launches on the step's tail: ds_grad_norms' two stages; ds_adam_tf_clipped
    replaces ds_adam_tf) -- two nets in ONE process, timed as interleaved pairs of windows (off, on, off, on, ...), device
    events around each window, every shape warmed up first, median / min / max of the windows;
  * with --parent-tree DIR: keys off against the package of another checkout (the parent commit, built in DIR), loaded into
    the same process under another module name and timed the same way -- the step without the keys must be the parent's step.

    python scripts/grad_clip_bench.py [--windows 5] [--iters 20] [--parent-tree DIR] [--out profiles/grad_clip.json]

Needs the GPU (no fallback).  bench.py (the flagship benchmark) is a different measurement and is not touched."""
import argparse
import importlib.util
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

DIMS = dict(mode="joint", nb_emotions=15, vocab_size=1000, embedding_dim=50, post_size=50)
BATCHES = (256, 32)
CLIP = 1.0


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
    return {"median": float(np.median(xs)), "min": xs[0], "max": xs[-1], "windows": xs}


def load_package(tree, name):
    """The package of another checkout under another module name (its relative imports and its own library stay its own)."""
    path = os.path.join(tree, "tumblr_emotions_amd")
    spec = importlib.util.spec_from_file_location(name, os.path.join(path, "__init__.py"), submodule_search_locations=[path])
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return importlib.import_module(name + ".net").SentimentNet, importlib.import_module(name + "._lib")


def interleaved(steps, windows, iters):
    """steps: {label: callable}.  Warm every one up, then `windows` rounds of one window each, in turn; the order rotates from
    round to round, so that no arm always runs behind the same neighbour."""
    for fn in steps.values():
        window_ms(fn, 3)
    ms = {k: [] for k in steps}
    order = list(steps)
    for w in range(windows):
        for k in order[w % len(order):] + order[:w % len(order)]:
            ms[k].append(window_ms(steps[k], iters))
    return {k: spread(v) for k, v in ms.items()}


def stepper(net, batch):
    return lambda: net.train_step(batch, 1e-4)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grad_clip.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "grad_clip_bench.py needs the GPU"
    _lib.load()
    ParentNet = None
    if args.parent_tree:
        ParentNet, parent_lib = load_package(os.path.abspath(args.parent_tree), "tumblr_emotions_amd_parent")
        parent_lib.load()
        assert os.path.realpath(parent_lib.LIB_PATH) != os.path.realpath(_lib.LIB_PATH)
    rows = []
    for B in BATCHES:
        batch = to_device(synthetic_batch_numpy(B, 50, 1000, seed=2))
        nets = {"off": SentimentNet(**DIMS), "clip_global_norm": SentimentNet(clip_global_norm=CLIP, **DIMS)}
        if ParentNet is not None:
            nets["parent"] = ParentNet(**DIMS)
        for net in nets.values():
            net.initialize(seed=1)
        iters = args.iters if B >= 128 else 3 * args.iters
        res = interleaved({k: stepper(n, batch) for k, n in nets.items()}, args.windows, iters)
        for k, n in nets.items():
            assert bool(torch.isfinite(n.store.theta).all()), k
        gn = nets["clip_global_norm"].grad_norms()
        st = nets["off"].store
        row = {"batch": B, "iters_per_window": iters, "step_ms": res,
               "clip_minus_off_ms": res["clip_global_norm"]["median"] - res["off"]["median"],
               "trainable_elements": int(st.n_trainable), "l2_elements": int(st.n_l2),
               "norm_pass_bytes": 4 * int(st.n_trainable_padded + st.n_l2),
               "segments": int(st.clip_segments.shape[0]), "chunks": int(st.clip_chunks.shape[0]),
               "last_global_norm": gn["global_norm"], "last_factor": gn["factor"]}
        if ParentNet is not None:
            p, o = res["parent"], res["off"]
            row["off_minus_parent_ms"] = o["median"] - p["median"]
            row["off_inside_parent_spread"] = bool(p["min"] <= o["median"] <= p["max"])
            same = all(torch.equal(getattr(nets["off"].store, x), getattr(nets["parent"].store, x)) for x in ("theta", "m", "v"))
            row["off_equals_parent_bit_for_bit"] = bool(same)
        rows.append(row)
        print(json.dumps(row), flush=True)
        del nets
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "model": "joint fp32, rnn_size 512, post_size 50, synthetic batch",
                   "clip_global_norm": CLIP, "method": "interleaved windows in one process, device events, %d windows" % args.windows,
                   "rows": rows}, f, indent=1)
    print("wrote", args.out)
