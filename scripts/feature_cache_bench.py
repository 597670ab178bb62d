"""What the Mixed_5b feature cache buys on the training step.  No dataset: random feature tensors go
straight into train_step.

  * the image step against the feature step -- joint and image model, fp32, frozen_bn + frozen betas, B = 256 and B = 32:
    two nets in ONE process, timed as interleaved windows (image, features, image, ...), device events around each window,
    every shape warmed up first, median / min / max of the windows.  The feature step includes its ds_rows_gather launch
    from a resident table, as the trainer runs it;
  * ds_rows_gather alone, over the trainer's six tables, against torch.index_select(..., out=) over the same tables (six
    launches) and against a device-to-device copy of the same bytes; achieved GB/s counts bytes read + bytes written;
  * with --parent-tree DIR: the step with the keys off (the default net) against the package of another checkout (the parent
    commit, built in DIR) loaded into the same process, timed the same way: without the keys the step must be the parent's.

    python scripts/feature_cache_bench.py [--windows 5] [--iters 20] [--parent-tree DIR] [--out profiles/feature_cache.json]

Needs the GPU (no fallback).  bench.py (the flagship benchmark) is a different measurement and is not touched."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from grad_clip_bench import interleaved, load_package      # noqa: E402
from tumblr_emotions_amd import _lib, ops                     # noqa: E402
from tumblr_emotions_amd.feature_cache import FEATURE_FLOATS, SMALL_KEYS      # noqa: E402
from tumblr_emotions_amd.net import SentimentNet              # noqa: E402
from tumblr_emotions_amd.synthetic import synthetic_batch_numpy, to_device      # noqa: E402

DIMS = {"joint": dict(mode="joint", nb_emotions=15, vocab_size=1000, embedding_dim=50, post_size=50),
        "image": dict(mode="image", nb_emotions=15)}
FROZEN = dict(frozen_bn=True, trainable_bn_beta=False)
BATCHES = (256, 32)
TABLE_ROWS = 2048            # 334 MB of features: past the 256 MiB Infinity Cache, so the gather reads HBM


def tables(batch, rows):
    """Resident tables of `rows` records (random features, the batch's small tensors tiled) and batch buffers of B rows."""
    B = batch["labels"].shape[0]
    src = {"features": torch.randn(rows, FEATURE_FLOATS, device="cuda")}
    for k in ("texts",) + SMALL_KEYS:
        reps = (-(-rows // B),) + (1,) * (batch[k].dim() - 1)
        src[k] = batch[k].repeat(*reps)[:rows].contiguous()
    dst = {k: torch.empty((B,) + tuple(v.shape[1:]), dtype=v.dtype, device="cuda") for k, v in src.items()}
    return src, dst


def feature_stepper(net, src, dst, perm, B, keys):
    """The trainer's step: ONE ds_rows_gather into the engine's Mixed_5b buffer and the batch buffers, then train_step."""
    state = {"at": 0, "gather": None, "ptr": None}
    order = ("features", "texts") + SMALL_KEYS

    def step():
        feat = net.feature_buffer(B)
        if state["ptr"] != feat.data_ptr():
            state["gather"] = ops.RowsGather([(src[k], feat.view(B, FEATURE_FLOATS) if k == "features" else dst[k]) for k in order])
            state["ptr"] = feat.data_ptr()
        lo = state["at"]
        state["at"] = (lo + B) % (perm.shape[0] - B + 1)
        state["gather"].run(perm[lo:lo + B])
        net.train_step(dict({k: dst[k] for k in keys}, features=feat), 1e-4)

    return step


def gather_alone(src, dst, perm, B, windows, iters):
    """The three arms on the same tables.  Every call takes the NEXT B entries of the permutation (the copy arm the next B
    rows), so a window walks the whole table -- 334 MB of features, past the Infinity Cache -- like a training pass does."""
    order = ("features", "texts") + SMALL_KEYS
    g = ops.RowsGather([(src[k], dst[k]) for k in order])
    slices = [perm[lo:lo + B] for lo in range(0, perm.shape[0] - B + 1, B)]
    at = {"ds_rows_gather": 0, "index_select": 0, "copy_same_bytes": 0}

    def turn(k):
        at[k] = (at[k] + 1) % len(slices)
        return at[k]

    def copy():
        lo = turn("copy_same_bytes") * B
        for k in order:
            dst[k].copy_(src[k][lo:lo + B])

    def select():
        idx = slices[turn("index_select")]
        for k in order:
            torch.index_select(src[k], 0, idx, out=dst[k])

    arms = {"ds_rows_gather": lambda: g.run(slices[turn("ds_rows_gather")]), "index_select": select, "copy_same_bytes": copy}
    res = interleaved(arms, windows, iters)
    moved = 2 * sum(dst[k].numel() * dst[k].element_size() for k in order)
    for k in arms:
        res[k]["gbytes_per_s"] = moved / (res[k]["median"] * 1e-3) / 1e9
    g.run(slices[0])
    for k in order:                                   # the gather leaves what fancy indexing gives
        assert torch.equal(dst[k], src[k][slices[0]]), k
    return dict(res, bytes_moved=moved, table_bytes=sum(v.numel() * v.element_size() for v in src.values()))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "feature_cache.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "feature_cache_bench.py needs the GPU"
    _lib.load()
    ParentNet = None
    if args.parent_tree:
        ParentNet, parent_lib = load_package(os.path.abspath(args.parent_tree), "tumblr_emotions_amd_parent")
        parent_lib.load()
        assert os.path.realpath(parent_lib.LIB_PATH) != os.path.realpath(_lib.LIB_PATH)
    rows = []
    for B in BATCHES:
        batch = to_device(synthetic_batch_numpy(B, 50, 1000, seed=2))
        src, dst = tables(batch, TABLE_ROWS)
        perm = torch.from_numpy(np.random.default_rng(1).permutation(TABLE_ROWS).astype(np.int64)).cuda()
        iters = args.iters if B >= 128 else 3 * args.iters
        row = {"batch": B, "iters_per_window": iters, "table_rows": TABLE_ROWS,
               "gather": gather_alone(src, dst, perm, B, args.windows, 10 * iters)}
        for mode in ("joint", "image"):
            keys = ("texts", "seq_lens", "labels") if mode == "joint" else ("labels",)
            a, b = SentimentNet(**FROZEN, **DIMS[mode]), SentimentNet(**FROZEN, **DIMS[mode])
            for net in (a, b):
                net.initialize(seed=1)
            image_batch = {k: batch[k] for k in ("images",) + keys}
            arms = {"image_step": lambda: a.train_step(image_batch, 1e-4),
                    "feature_step": feature_stepper(b, src, dst, perm, B, keys)}
            res = interleaved(arms, args.windows, iters)
            for net in (a, b):
                assert bool(torch.isfinite(net.store.theta).all())
            row[mode] = {"step_ms": res, "image_over_feature": res["image_step"]["median"] / res["feature_step"]["median"]}
            del a, b, arms
            torch.cuda.empty_cache()
        if ParentNet is not None:        # keys absent: this tree's default step against the parent commit's
            nets = {"off": SentimentNet(**DIMS["joint"]), "parent": ParentNet(**DIMS["joint"])}
            for net in nets.values():
                net.initialize(seed=1)
            full = {k: batch[k] for k in ("images", "texts", "seq_lens", "labels")}
            res = interleaved({k: (lambda n=n: n.train_step(full, 1e-4)) for k, n in nets.items()}, args.windows, iters)
            p, o = res["parent"], res["off"]
            same = all(torch.equal(getattr(nets["off"].store, x), getattr(nets["parent"].store, x)) for x in ("theta", "m", "v"))
            row["keys_off"] = {"step_ms": res, "off_minus_parent_ms": o["median"] - p["median"],
                               "off_inside_parent_spread": bool(p["min"] <= o["median"] <= p["max"]),
                               "off_equals_parent_bit_for_bit": bool(same)}
            del nets
            torch.cuda.empty_cache()
        rows.append(row)
        print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0),
                   "model": "fp32, frozen_bn + trainable_bn_beta=False, rnn_size 512, post_size 50, synthetic batch, random features",
                   "method": "interleaved windows in one process, device events, %d windows" % args.windows, "rows": rows}, f, indent=1)
    print("wrote", args.out)
