#!/usr/bin/env python
"""Input gradients, measured: the stem's Conv2DBackpropInput (ds_conv_stem_dgrad, through ds_conv_run) at B = 1, 32, 256
next to the forward stem (ds_conv_stem) at the same B -- us per launch and TFLOP/s of the algorithmic work (2 N OH OW 64 147,
the same for both) -- then the wall time of one SentimentNet.input_gradient (image and joint mode) at B = 1 and 32, and of
one class_visualisation iteration (difference of a 102- and a 2-iteration run on a synthetic checkpoint, B = 1).
Prints one JSON line per measurement.  Each part can be run alone: `input_grad_bench.py kernel|model|vis`."""
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from tumblr_emotions_amd import ops

PEAK_F32 = 157.3e12        # fp32 (MFMA and v_pk_fma_f32) peak of the MI355X, FLOP/s


def timeit(f, reps=20):
    for _ in range(3):
        f()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


def wall(f, reps=10):
    f()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def kernel():
    for B in (1, 32, 256):
        x = torch.rand(B, 224, 224, 3, device="cuda") * 2 - 1
        w = torch.randn(7, 7, 4, 64, device="cuda") * 0.1
        fwd = ops.LayerPlan(ops.DS_CONV_FWD, ops.DS_ARITH_F32, ops.DS_PLAN_PACKED_RGB, B, 224, 224, 4, 64, 7, 2, 4, 64,
                            ops.DS_EPI_STATS)
        z = torch.empty(fwd.M, 64, device="cuda")
        stats = torch.zeros(2 * 64 * max(fwd.partials, 1), device="cuda")
        pivot = torch.zeros(64, device="cuda")
        dg = ops.LayerPlan(ops.DS_CONV_DGRAD, ops.DS_ARITH_F32, ops.DS_PLAN_PACKED_RGB, B, 224, 224, 4, 64, 7, 2, 64, 3, 0)
        dx = torch.empty(B, 224, 224, 3, device="cuda")
        t_f = timeit(lambda: fwd.run(ops._p(x), ops._p(w), ops._p(z), stats=ops._p(stats), pivot=ops._p(pivot)))
        t_d = timeit(lambda: dg.run(ops._p(z), ops._p(w), ops._p(dx)))
        fl = dg.alg_flops
        print(json.dumps({"what": "stem", "B": B, "gflop": round(fl / 1e9, 3),
                          "fwd_us": round(t_f, 1), "fwd_tflops": round(fl / t_f / 1e6, 1),
                          "fwd_of_peak": round(fl / t_f / 1e6 / (PEAK_F32 / 1e12), 3),
                          "dgrad_us": round(t_d, 1), "dgrad_tflops": round(fl / t_d / 1e6, 1),
                          "dgrad_of_peak": round(fl / t_d / 1e6 / (PEAK_F32 / 1e12), 3)}), flush=True)


def model():
    from tumblr_emotions_amd.net import SentimentNet
    from tumblr_emotions_amd.synthetic import synthetic_batch_numpy, to_device
    for mode in ("image", "joint"):
        kw = dict(vocab_size=1000, embedding_dim=50, post_size=50) if mode == "joint" else {}
        net = SentimentNet(mode=mode, nb_emotions=15, **kw)
        net.initialize(seed=1)
        for B in (1, 32):
            batch = to_device(synthetic_batch_numpy(B, 50, 1000, seed=B))
            t = wall(lambda: net.input_gradient(batch, 3))
            print(json.dumps({"what": "input_gradient", "mode": mode, "B": B, "ms": round(t, 2)}), flush=True)
        del net
        torch.cuda.empty_cache()


def vis():
    from tumblr_emotions_amd.image_text_model import im_text_rnn_model as M
    cfg = dict(synthetic=True, batch_size=4, num_samples=8, vocab_size=1000, embedding_dim=50, post_size=50)
    with tempfile.TemporaryDirectory() as d:
        ckpt = os.path.join(d, "ckpt")
        M.train_deep_sentiment(None, ckpt, 1, config=cfg, quiet=True)
        M.class_visualisation(0, 100.0, ckpt, config=cfg, num_iterations=2, out_dir=os.path.join(d, "out"))      # (warm-up)
        ts = {}
        for n in (2, 102):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            M.class_visualisation(0, 100.0, ckpt, config=cfg, num_iterations=n, out_dir=os.path.join(d, "out"))
            torch.cuda.synchronize()
            ts[n] = time.perf_counter() - t0
        print(json.dumps({"what": "class_visualisation_iteration", "B": 1, "ms": round((ts[102] - ts[2]) / 100 * 1e3, 2)}),
              flush=True)


if __name__ == "__main__":
    parts = sys.argv[1:] or ["kernel", "model", "vis"]
    for p in parts:
        {"kernel": kernel, "model": model, "vis": vis}[p]()
