"""Fused inference forward on the GPU: BatchNorm + ReLU in the conv epilogue (DS_EPI_BN_RELU) against today's
conv -> ds_bn_apply_relu, BIT FOR BIT (torch.equal; tolerance zero: both sites are one fp32 fused multiply-add and a max
on the same accumulators), per layer, per model, with its invalidation, launch counts and the front ends."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from oracle import tf_semantics as S

pytestmark = pytest.mark.gpu

SMALL = dict(batch_size=4, rnn_size=32, vocab_size=60, embedding_dim=20, post_size=12, num_samples=12, synthetic=True)


def _net(mode, steps=3, B=6, seed=5):
    """A net whose moving statistics and betas have left their initial values (a few train steps)."""
    from tumblr_emotions_amd.net import SentimentNet
    kw = dict(nb_emotions=15) if mode == "image" else dict(nb_emotions=15, im_features_size=256, rnn_size=32, fc_size=512,
                                                            vocab_size=50, embedding_dim=16, post_size=8)
    net = SentimentNet(mode=mode, **kw)
    net.initialize(seed=seed)
    for i in range(steps):
        net.train_step(_batch(B, seed + i), 1e-3)
    torch.cuda.synchronize()
    return net


def _batch(B, seed):
    b = S.synthetic_batch(B, 8, 50, seed=seed)
    return {k: torch.from_numpy(v).cuda() for k, v in b.items() if k in ("images", "texts", "seq_lens", "labels")}


def _both(net, batch):
    a = net.predict(batch, is_training=False, fused=False).clone()
    b = net.predict(batch, is_training=False, fused=True).clone()
    c = net.predict(batch, is_training=False, fused=False).clone()
    torch.cuda.synchronize()
    return a, b, c


# ---- per layer ------------------------------------------------------------------------------------------------------------
def _copy(src, keep_pool):
    from tumblr_emotions_amd import _lib
    q = _lib.LayerPlanStruct()
    C.memmove(C.addressof(q), C.addressof(src), C.sizeof(q))
    d = q.d
    d.norm_rstd = d.norm_shift = d.mask_rstd = d.mask_shift = None
    d.bnb = None
    if not keep_pool:
        d.pool_argmax = None
    _lib.load().ds_conv_plan_set_flags(C.byref(q), 0)
    return q


@pytest.mark.parametrize("N", [1, 32, 256])
def test_every_forward_plan_fused_equals_conv_then_apply(N):
    from tumblr_emotions_amd import _lib, ops
    from tumblr_emotions_amd.net import SentimentNet
    lib = _lib.load()
    net = SentimentNet(mode="image", nb_emotions=15)
    net.initialize(seed=1)
    net.predict(_batch(N, 3), is_training=False)
    torch.cuda.synchronize()
    plans = [(l.key, l.fwd.p, l.cin, l.cout, l.k, l.H, l.W) for l in net.image.layers if not l.fold]
    assert len(plans) == 38          # 57 convs = the stem + 2 + 9 x (one launch for three 1x1 convs, two 3x3, Branch_3 1x1)
    gen = torch.Generator(device="cuda").manual_seed(N)
    st = ops._stream()
    fams = set()
    for key, src, cin, cout, k, H, W in plans:
        pooled = bool(src.d.pool_argmax)
        M = N * H * W
        x = torch.rand(N, H, W, cin, device="cuda", generator=gen) * 2 - 1
        w = (torch.rand(k, k, cin, cout, device="cuda", generator=gen) * 2 - 1) * (1.0 / (k * np.sqrt(cin)))
        scale = torch.rand(cout, device="cuda", generator=gen) * 9.9 + 0.1
        shift = torch.rand(cout, device="cuda", generator=gen) * 2 - 1
        shift[0] = -1e4                                   # a channel the ReLU clamps everywhere
        argmax = torch.zeros(M, cin, dtype=torch.uint8, device="cuda") if pooled else None
        pad, ld, rows = 8, cout + 24, M + 5               # destination: columns [8, 8 + cout) of rows [0, M)
        outs = []
        for fused in (False, True):
            q = _copy(src, pooled)
            q.d.ldx = cin
            if pooled:
                q.d.pool_argmax = argmax.data_ptr()
            io = _lib.ConvIO()
            ws = torch.empty(max(int(q.ws_bytes) // 4, 4), device="cuda")
            io.ws, io.ws_bytes = ws.data_ptr(), ws.numel() * 4
            u = torch.empty(int(q.w_bytes), dtype=torch.uint8, device="cuda") if q.w_bytes else None
            if u is not None:
                assert lib.ds_conv_prepare_weights(C.byref(q), ops._p(w), ops._p(u), None, st) == 0
            wp = ops._p(u if u is not None else w)
            dest = torch.full((rows, ld), -7.0, device="cuda")
            dptr = C.c_void_p(dest.data_ptr() + 4 * pad)
            if fused:
                assert lib.ds_conv_plan_enable_bn_relu(C.byref(q)) == 1, key
                q.d.ldz = ld
                io.scale, io.shift = scale.data_ptr(), shift.data_ptr()
                assert lib.ds_conv_run(C.byref(q), ops._p(x), wp, dptr, C.byref(io), st) == 0, lib.ds_last_error()
                fams.add((q.family, q.splitk > 1, pooled))
            else:
                z = torch.empty(M, cout, device="cuda")
                q.d.ldz = cout
                assert lib.ds_conv_run(C.byref(q), ops._p(x), wp, ops._p(z), C.byref(io), st) == 0, lib.ds_last_error()
                ops.bn_apply_relu(z, M, cout, scale, shift, ops.make_segments([(0, cout, dptr.value, ld)]))
            torch.cuda.synchronize()
            outs.append(dest)
        a, b = outs
        assert torch.equal(a, b), (key, N, float((a - b).abs().max()))
        assert float(b[:M, pad].max()) == 0.0 and float(b[:M, pad:pad + cout].max()) > 0.0
        assert bool((b[M:] == -7.0).all()) and bool((b[:, :pad] == -7.0).all()) and bool((b[:, pad + cout:] == -7.0).all())
    print("families (family, split-K, pool on load) at N = %d: %s" % (N, sorted(fams)))
    assert any(f[0] == _lib.DS_FAM_IGEMM for f in fams) and any(f[0] == _lib.DS_FAM_WINO4 for f in fams)


def test_prepare_multi_equals_per_layer_prepare():
    from tumblr_emotions_amd import ops
    net = _net("image", steps=2)
    net.predict(_batch(2, 1), is_training=False)
    layers = net.image.layers
    assert sum(len(l.scopes) for l in layers) == 57
    want, jobs, got = [], [], []
    for l in layers:
        r, s = torch.empty(l.cout, device="cuda"), torch.empty(l.cout, device="cuda")
        ops.bn_infer_prepare(l.beta, l.mm, l.mv, 1e-3, l.cout, r, s)
        want.append((r, s))
        r2, s2 = torch.full((l.cout,), 9.0, device="cuda"), torch.full((l.cout,), 9.0, device="cuda")
        jobs.append((l.beta, l.mm, l.mv, l.cout, r2, s2))
        got.append((r2, s2))
    ops.BnInferJobs(jobs).run(1e-3)
    torch.cuda.synchronize()
    for (r, s), (r2, s2) in zip(want, got):
        assert torch.equal(r, r2) and torch.equal(s, s2)


# ---- model ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["image", "joint"])
def test_fused_predict_equals_unfused_bit_for_bit(mode):
    net = _net(mode)
    for B in (1, 5, 32, 256):
        a, b, c = _both(net, _batch(B, 100 + B))
        assert torch.equal(a, b) and torch.equal(a, c), (mode, B, float((a - b).abs().max()))
        assert bool(torch.isfinite(b).all()) and float(b.abs().max()) > 0
    batch = _batch(5, 7)
    f0 = net.predict(batch, fused=True).clone()
    net.train_step(_batch(6, 50), 1e-3)                   # beta and the moving statistics move: the prepared vectors are stale
    a, b, _ = _both(net, batch)
    assert torch.equal(a, b) and not torch.equal(b, f0)
    sd = net.state_dict()
    rng = np.random.RandomState(3)
    for k in sd:
        if k.endswith("moving_mean"):
            sd[k] = sd[k] + rng.normal(0, 0.05, size=sd[k].shape).astype(sd[k].dtype)
    f1 = net.predict(batch, fused=True).clone()
    net.load_state_dict(sd)
    a, b, _ = _both(net, batch)
    assert torch.equal(a, b) and not torch.equal(b, f1)


def _step_after(predicts):
    """State after one train step that follows `predicts` = [(batch size, fused)] on a freshly trained net."""
    net = _net("joint", steps=2, seed=11)
    for B, fused in predicts:
        net.predict(_batch(B, 70 + B), is_training=False, fused=fused)
    net.train_step(_batch(6, 20), 1e-3)
    torch.cuda.synchronize()
    return net.state_dict(), net.store.m.clone(), net.store.v.clone()


def _same_state(x, y):
    (sa, ma, va), (sb, mb, vb) = x, y
    assert sorted(sa) == sorted(sb)
    for k in sa:
        np.testing.assert_array_equal(sa[k], sb[k], err_msg=k)
    assert torch.equal(ma, mb) and torch.equal(va, vb)


def test_a_fused_predict_leaves_the_next_train_step_unchanged():
    """Variables (moving statistics included) and Adam slots after a train step, bitwise: with two fused predicts in front of
    it against none.  The predicts use the training batch size: a predict at ANOTHER batch size re-allocates the engine, which
    resets the BatchNorm statistics pivots to the moving means (ConvBN.bind) -- fused or not, and before this feature -- and
    that moves the next step's batch statistics in their last bits.  That case is held against the same sequence with unfused
    predicts instead: the fused pass adds nothing to it."""
    _same_state(_step_after([]), _step_after([(6, True), (6, True)]))
    _same_state(_step_after([(3, False), (6, False)]), _step_after([(3, True), (6, True)]))


def test_fused_report_and_launch_counts(monkeypatch):
    from tumblr_emotions_amd import ops
    net = _net("image", steps=1)
    batch = _batch(32, 9)
    net.predict(batch, fused=True)
    report = net.fused_report()
    print("fused_report:", report)
    layers = {l.key: l for l in net.image.layers}
    # Every 1x1 and 3x3 layer with ONE destination carries the epilogue.  The only 1x1 launches allowed in the report are the
    # horizontally fused block-input convs, whose output scatters to three destinations (Branch_0's concat slice and the two
    # reduce buffers): the case the feature's specification itself sends to conv -> apply; they must say so.
    for k, reason in report:
        if layers[k].k in (1, 3):
            assert k.endswith("/fused_1x1") and "3 destinations" in reason, (k, reason)
    assert sum(1 for k, _ in report if layers[k].k in (1, 3)) <= 9 and len(report) <= 10, report
    assert not any(layers[k].k == 3 for k, _ in report), report
    calls = {"prepare": 0, "apply": 0, "fused": 0, "plain": 0}
    order = []

    def count(name, fn):
        def wrapped(*a, **kw):
            calls[name] += 1
            order.append(name)
            return fn(*a, **kw)
        return wrapped
    monkeypatch.setattr(ops, "bn_infer_prepare", count("prepare", ops.bn_infer_prepare))
    monkeypatch.setattr(ops.BnInferJobs, "run", count("prepare", ops.BnInferJobs.run))
    monkeypatch.setattr(ops, "bn_apply_relu", count("apply", ops.bn_apply_relu))
    monkeypatch.setattr(ops.LayerPlan, "run_bn_relu", count("fused", ops.LayerPlan.run_bn_relu))
    monkeypatch.setattr(ops.LayerPlan, "run", count("plain", ops.LayerPlan.run))
    net.predict(batch, fused=True)
    # 39 conv launches: 29 with the epilogue (Conv2d_2b, 2c and the three block-closing convs of the nine Mixed blocks), the
    # stem and the nine three-destination launches without; an apply pass only behind a launch without it; nothing prepared
    print("fused launches:", calls)
    assert calls["prepare"] == 0
    assert calls["fused"] == 29 and calls["plain"] == 10 == len(report), calls
    assert calls["apply"] <= len(report)
    for i, name in enumerate(order):
        if name == "apply":
            assert order[i - 1] == "plain", order[max(0, i - 3):i + 1]
    # the unfused pass on the same net: every conv plain, one prepare per layer
    for k in calls:
        calls[k] = 0
    net.predict(batch, fused=False)
    print("unfused launches:", calls)
    assert calls["fused"] == 0 and calls["plain"] == 39 and calls["prepare"] == 39, calls


# ---- front ends -----------------------------------------------------------------------------------------------------------
def test_front_ends_give_identical_results_with_fused_inference(tmp_path, monkeypatch):
    from tumblr_emotions_amd.image_text_model import im_text_rnn_model as M
    from tumblr_emotions_amd.net import SentimentNet
    seen = []
    real = SentimentNet.predict

    def spy(self, batch, is_training=False, seed=None, fused=False):
        out = real(self, batch, is_training=is_training, seed=seed, fused=fused)
        seen.append((is_training, fused, bool(fused) and len(self.fused_report()) > 0))
        return out
    monkeypatch.setattr(SentimentNet, "predict", spy)
    ckpt = str(tmp_path / "joint")
    M.train_deep_sentiment(None, ckpt, 2, config=SMALL, quiet=True)
    res = []
    for tag, cfg in (("plain", SMALL), ("fused", dict(SMALL, fused_inference=True))):
        on = tag == "fused"
        out = str(tmp_path / ("data_" + tag))
        del seen[:]
        acc = M.evaluate_deep_sentiment(ckpt, str(tmp_path / ("log_" + tag)), "validation", 3, config=cfg, quiet=True)
        assert seen == [(False, on, on)] * 3, seen          # the key reaches predict, and the engine ran its fused pass
        del seen[:]
        acc_t = M.evaluate_deep_sentiment(ckpt, str(tmp_path / ("log_" + tag)), "train", 1, config=cfg, quiet=True)
        assert seen == [(True, False, False)], seen         # mode 'train' keeps batch statistics: the key is ignored
        del seen[:]
        M.day_of_week_trend(ckpt, config=cfg, out_dir=out)
        assert len(seen) >= 1 and all(x == (False, on, on) for x in seen), seen
        res.append((acc, acc_t, {f: np.load(os.path.join(out, f)) for f in sorted(os.listdir(out)) if f.endswith(".npy")}))
    (a0, t0, f0), (a1, t1, f1) = res
    assert a0 == a1 and 0.0 <= t1 <= 1.0
    assert sorted(f0) == sorted(f1) and len(f0) >= 1
    for k in f0:
        np.testing.assert_array_equal(f0[k], f1[k], err_msg=k)
