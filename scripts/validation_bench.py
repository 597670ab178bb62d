"""What streaming metrics and validation during training cost, measured on the MI355X in ONE process with alternating windows.

(a) ms per evaluation batch of training.run_evaluation at batch 256 -- the text model and the joint fp32 model with
    config['fused_inference'] -- in three arms: config['eval_metrics'] (metrics.StreamingMetrics: one ds_eval_metrics_update
    per batch, one read-back at the end), without the key (argmax + .sum() + .item() per batch), and `parent_loop`, the
    evaluation loop as it stood before the key existed, restated below (the arm without the key runs the same lines).
    run_evaluation also restores the checkpoint and writes its lines, so a window times it at two lengths and divides the
    difference: (t(long) - t(short)) / (long - short).  The batches are built once and stay on the device (batch_fn).
(b) training samples/s of the joint model over --train-steps steps (300) of training.run_training at batch 256, with
    validate_every=100, validate_batches=10 and without, host clock around the whole call (it ends in the checkpoint's
    synchronise); the training batches stay on the device (batch_fn), the validation batches are built before the clock
    starts and that one-off time is reported beside the rates.

    python scripts/validation_bench.py [--windows 5] [--train-steps 300] [--out profiles/validation.json]

Every arm is warmed up first; the spread of the windows is reported next to their median.  Needs the GPU (no fallback).
bench.py (the flagship benchmark) is a different measurement and is not touched."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tumblr_emotions_amd import _lib, training                                     # noqa: E402
from tumblr_emotions_amd.synthetic import synthetic_batch_numpy, to_device         # noqa: E402

B, T, V, D, H = 256, 32, 10000, 300, 512
TEXT = dict(batch_size=B, rnn_size=H, vocab_size=V, embedding_dim=D, post_size=T, num_samples=50000, synthetic=True)


def spread(xs):
    xs = sorted(xs)
    return {"median": float(np.median(xs)), "min": xs[0], "max": xs[-1]}


def parent_loop(model, checkpoint_dir, log_dir, mode, num_evals, batch_fn):
    """run_evaluation before config['eval_metrics'] existed."""
    step = training.load_checkpoint(model, training.latest_checkpoint(checkpoint_dir))
    is_training = mode == "train"
    fused = bool(model.config.get("fused_inference", False)) and not is_training
    correct = total = 0
    for i in range(num_evals):
        batch = batch_fn(i)
        logits = model.net.predict(batch, is_training=is_training, fused=fused)
        model.logits, model.labels = logits, batch["labels"]
        correct += int((logits.argmax(dim=1) == batch["labels"]).sum().item())
        total += int(batch["labels"].shape[0])
    acc = correct / max(total, 1)
    out_dir = os.path.join(log_dir, mode)
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "accuracy.jsonl"), "a") as f:
        f.write(json.dumps({"global_step": step, "accuracy": acc, "num_evals": num_evals, "mode": mode}) + "\n")
    return acc


def make_model(kind, extra):
    if kind == "text":
        from tumblr_emotions_amd.text_model.text_embedding import _CONFIG, TextModel
        return TextModel(dict(_CONFIG, **dict(TEXT, **extra)))
    from tumblr_emotions_amd.image_text_model.im_text_rnn_model import _CONFIG, DeepSentiment
    return DeepSentiment(dict(_CONFIG, **dict(TEXT, fused_inference=True, **extra)))


def evaluation_bench(kind, windows, short, long, work):
    batches = [to_device(synthetic_batch_numpy(B, T, V, seed=10 ** 6 + i, with_images=(kind == "joint"))) for i in range(4)]
    batch_fn = lambda i: batches[i % len(batches)]                          # noqa: E731
    ckpt, log = os.path.join(work, kind + "_ckpt"), os.path.join(work, kind + "_log")
    os.makedirs(ckpt)
    models = {"eval_metrics": make_model(kind, {"mode": "validation", "eval_metrics": True}),
              "without_key": make_model(kind, {"mode": "validation"})}
    models["parent_loop"] = models["without_key"]
    for i in range(2):                                                      # moving statistics off their initial values
        models["without_key"].net.train_step(batches[i], 1e-3)
    training.save_checkpoint(models["without_key"], ckpt, 2)

    def timed(arm, n):
        m = models[arm]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if arm == "parent_loop":
            acc = parent_loop(m, ckpt, log, "validation", n, batch_fn)
        else:
            acc = training.run_evaluation(m, ckpt, log, "validation", n, batch_fn=batch_fn, quiet=True)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, acc

    arms = ("eval_metrics", "without_key", "parent_loop")
    accs = {arm: timed(arm, short)[1] for arm in arms}                      # warm-up, and the three arms agree
    assert len(set(accs.values())) == 1, accs
    ms = {arm: [] for arm in arms}
    for _ in range(windows):
        for arm in arms:
            ms[arm].append(1e3 * (timed(arm, long)[0] - timed(arm, short)[0]) / (long - short))
    out = {"model": kind, "batch": B, "fused_inference": kind == "joint", "evals_short": short, "evals_long": long,
           "windows": windows, "accuracy": accs["eval_metrics"],
           "ms_per_eval_batch": {arm: spread(ms[arm]) for arm in arms}}
    out["eval_metrics_over_parent_median"] = (out["ms_per_eval_batch"]["eval_metrics"]["median"]
                                              / out["ms_per_eval_batch"]["parent_loop"]["median"])
    del models, batches
    torch.cuda.empty_cache()
    return out


def training_bench(windows, steps, work):
    batches = [to_device(synthetic_batch_numpy(B, T, V, seed=i)) for i in range(2)]
    batch_fn = lambda step: batches[step % len(batches)]                    # noqa: E731
    models = {"validate_every_100": make_model("joint", {"validate_every": 100, "validate_batches": 10}),
              "without_key": make_model("joint", {})}
    t0 = time.perf_counter()
    n_valid = len(list(models["validate_every_100"].validation_batches(10)))
    torch.cuda.synchronize()
    build_s = time.perf_counter() - t0

    def timed(arm, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        training.run_training(models[arm], os.path.join(work, "train_" + arm), n, batch_fn=batch_fn, log_every=100, quiet=True)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    for arm in models:
        timed(arm, 10)                                                      # warm-up: every shape, one validation
    rate = {arm: [] for arm in models}
    for _ in range(windows):
        for arm in models:
            rate[arm].append(steps * B / timed(arm, steps))
    lines = [json.loads(l) for l in open(os.path.join(work, "train_validate_every_100", "validation.jsonl"))]
    out = {"model": "joint", "batch": B, "fused_inference": True, "steps": steps, "windows": windows,
           "validations_per_run": len(lines), "validation_batches": n_valid, "validation_batches_build_s": build_s,
           "samples_per_s": {arm: spread(rate[arm]) for arm in models}}
    out["validated_over_plain_median"] = (out["samples_per_s"]["validate_every_100"]["median"]
                                          / out["samples_per_s"]["without_key"]["median"])
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--evals", type=int, nargs=2, default=(8, 40), metavar=("SHORT", "LONG"))
    ap.add_argument("--train-steps", type=int, default=300)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "validation.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "validation_bench.py needs the GPU"
    _lib.load()
    result = {"device": torch.cuda.get_device_name(0), "evaluation": []}
    with tempfile.TemporaryDirectory() as work:
        for kind in ("text", "joint"):
            r = evaluation_bench(kind, args.windows, args.evals[0], args.evals[1], work)
            result["evaluation"].append(r)
            print("%-5s ms per eval batch: %s" % (kind, {k: round(v["median"], 4) for k, v in r["ms_per_eval_batch"].items()}),
                  flush=True)
        result["training"] = training_bench(args.windows, args.train_steps, work)
        print("training samples/s: %s" % {k: round(v["median"], 1) for k, v in result["training"]["samples_per_s"].items()},
              flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", args.out)
