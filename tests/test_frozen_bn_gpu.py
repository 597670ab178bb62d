"""Frozen-BatchNorm training on the device (SentimentNet(frozen_bn=True)): the three new kernels against their
siblings and against fp64 sums, and the whole step against the fp64 reference of tests/test_frozen_bn_cpu.py."""
import os
import socket

import numpy as np
import pytest
import torch

from oracle import tf_semantics as S
from oracle import torch_ref as R
from test_frozen_bn_cpu import FrozenBNRef

pytestmark = pytest.mark.gpu

SENTINEL = -777.25
U = 2.0 ** -24


def _cuda(a, dtype=torch.float32):
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


# ---- kernels --------------------------------------------------------------------------------------------------------------
#                M,   C, ldz, dy layout
POINTWISE = [(1, 16, 16, "one"),
             (147, 24, 24, "one"),
             (392, 208, 512, "three"),
             (1568, 96, 480, "one"),
             (5, 1040, 1040, "one")]          # (beyond the net's widths: C / 4 > 256, a workgroup meets only some column groups)


def _pointwise_inputs(M, C, ldz, layout, integer, seed):
    """z [M, ldz] with sentinels outside [0, C); rstd > 0, shift; dy as ds_segments over their own strided buffers (sentinels
    between the rows' ends), as one dense [M, C] fp32 tensor."""
    from tumblr_emotions_amd import ops
    rng = np.random.RandomState(seed)
    z = np.full((M, ldz), SENTINEL, np.float32)
    z[:, :C] = rng.normal(0, 1, size=(M, C))
    rstd = rng.uniform(0.5, 2.0, size=C).astype(np.float32)
    shift = rng.normal(0, 0.5, size=C).astype(np.float32)
    draw = (lambda shape: rng.randint(-8, 9, size=shape).astype(np.float32)) if integer else \
        (lambda shape: rng.normal(0, 1, size=shape).astype(np.float32))
    cuts = {"one": [0, C], "three": [0, 64, 160, C]}[layout]
    keep, parts, dense = [], [], np.zeros((M, C), np.float32)
    for i, (c0, c1) in enumerate(zip(cuts[:-1], cuts[1:])):
        ld = (c1 - c0) + 4 * (i + 1)
        buf = np.full((M, ld), SENTINEL, np.float32)
        buf[:, :c1 - c0] = draw((M, c1 - c0))
        dense[:, c0:c1] = buf[:, :c1 - c0]
        t = _cuda(buf)
        keep.append(t)
        parts.append((c0, c1, t.data_ptr(), ld))
    segs = ops.make_segments(parts)
    return _cuda(z), _cuda(rstd), _cuda(shift), segs, keep, dense


def _reduce(partials, P, C, n_layers=1):
    """ds_bn_dbeta_reduce_multi over `n_layers` column ranges of one partials tensor -> [C] on the host."""
    from tumblr_emotions_amd import ops
    out = torch.full((C + 8,), SENTINEL, device="cuda")
    edges = [C * i // n_layers // 4 * 4 for i in range(n_layers)] + [C]
    jobs = [(partials.data_ptr() + 4 * c0 * P, P, c1 - c0, out[c0:c1]) for c0, c1 in zip(edges[:-1], edges[1:])]
    ops.BnSumJobs(jobs).run()
    torch.cuda.synchronize()
    assert bool((out[C:] == SENTINEL).all())
    return out[:C].cpu().numpy()


@pytest.mark.parametrize("M,C,ldz,layout", POINTWISE, ids=["%dx%d_ld%d_%s" % c for c in POINTWISE])
def test_pointwise_kernel_writes_the_siblings_dz_and_exact_column_sums(M, C, ldz, layout):
    from tumblr_emotions_amd import ops
    P = ops.bn_infer_bwd_partials(M, C)
    assert P >= 1
    if M == 1568:
        assert P > 1
    for integer in (True, False):
        z, rstd, shift, segs, keep, dense = _pointwise_inputs(M, C, ldz, layout, integer, seed=M + C + integer)
        want = torch.full((M, ldz), SENTINEL, device="cuda")
        ops.bn_infer_bwd_apply(z, segs, M, C, rstd, shift, want, ldz=ldz)
        # the predicate as the sibling evaluates it: its dz for dy = 1 is rstd * [z*rstd + shift > 0], and rstd > 0
        ones = torch.ones(M, C, device="cuda")
        probe = torch.zeros(M, ldz, device="cuda")
        ops.bn_infer_bwd_apply(z, ops.make_segments([(0, C, ones.data_ptr(), C)]), M, C, rstd, shift, probe, ldz=ldz)
        torch.cuda.synchronize()
        on = (probe[:, :C] != 0).cpu().numpy()
        assert on.any() and not on.all()
        g = np.where(on, dense, np.float32(0)).astype(np.float64)
        exact = g.sum(0)

        guard = 64
        for alias in (False, True):
            part = torch.full((C * P + guard,), SENTINEL, device="cuda")
            if alias:
                dz = z.clone()
                ops.bn_infer_bwd_apply_sums(dz, segs, M, C, rstd, shift, dz, part, ldz=ldz)
            else:
                dz = torch.full((M, ldz), SENTINEL, device="cuda")
                zin = z.clone()
                ops.bn_infer_bwd_apply_sums(zin, segs, M, C, rstd, shift, dz, part, ldz=ldz)
            torch.cuda.synchronize()
            assert torch.equal(dz[:, :C], want[:, :C]), "dz differs from ds_bn_infer_bwd_apply (alias=%s)" % alias
            assert bool((dz[:, C:] == SENTINEL).all()), "columns outside [0, C) written"
            if not alias:
                assert torch.equal(zin, z)
            assert bool((part[C * P:] == SENTINEL).all()) and bool((part[:C * P] != SENTINEL).all())
            for seg_buf in keep:                                     # the gradient segments are read-only
                assert bool((seg_buf[:, -4:] == SENTINEL).all())
            for n_layers in (1, 3):
                got = _reduce(part, P, C, n_layers).astype(np.float64)
                err = np.abs(got - exact)
                bound = 0.0 if integer else (M - 1) * U * np.abs(g).sum(0)
                print("M=%d C=%d %s integer=%s alias=%s layers=%d: max error %.3e (bound min %.3e)"
                      % (M, C, layout, integer, alias, n_layers, err.max(), np.min(bound)))
                assert (err <= bound).all()
        # sums only (dz NULL): the same partial sums, nothing else written
        part2 = torch.full((C * P + guard,), SENTINEL, device="cuda")
        zin = z.clone()
        ops.bn_infer_bwd_apply_sums(zin, segs, M, C, rstd, shift, None, part2, ldz=ldz)
        torch.cuda.synchronize()
        assert torch.equal(zin, z) and torch.equal(part2, part)


POOLED = [(N, H, W, C) for N in (1, 2) for (H, W) in ((8, 8), (7, 9)) for C in (64, 192)]


@pytest.mark.parametrize("N,H,W,C", POOLED, ids=["%dx%dx%dx%d" % c for c in POOLED])
def test_pooled_twin_writes_the_siblings_dz_and_exact_column_sums(N, H, W, C):
    """conv -> BatchNorm -> ReLU -> 3x3/2 pool from the POOLED gradient, on tie-rich z (multiples of 0.25: duplicated window
    maxima, winners decided by the arg-max record).  rstd is a power of two here, so g = dz / rstd exactly."""
    from tumblr_emotions_amd import ops
    rng = np.random.RandomState(N * 1000 + H * 100 + W * 10 + C)
    z = _cuda(np.round(rng.normal(0, 0.3, size=(N, H, W, C)) * 4) / 4)
    rstd = _cuda(2.0 ** rng.randint(-1, 3, size=C))
    shift = _cuda(np.round(rng.normal(0, 0.2, size=C) * 4) / 4)
    OH, OW = (H + 1) // 2, (W + 1) // 2
    y = torch.empty(N, OH, OW, C, device="cuda")
    am = torch.empty(N, OH, OW, C, dtype=torch.uint8, device="cuda")
    assert ops.maxpool_bn_relu_fwd(z, rstd, shift, y, am, N, H, W, C, 3, 2) == (OH, OW)
    P = ops.bn_pool_bwd_partials(N, H, W, C)
    M = N * H * W
    for integer in (True, False):
        dpool = _cuda(rng.randint(-8, 9, size=(N, OH, OW, C)) if integer else rng.normal(0, 1, size=(N, OH, OW, C)))
        want = torch.empty_like(z)
        ops.bn_pool_infer_bwd_apply(z, dpool, am, N, H, W, C, rstd, shift, want)
        torch.cuda.synchronize()
        g = (want / rstd).cpu().numpy().reshape(M, C).astype(np.float64)
        assert (g != 0).any()
        exact = g.sum(0)
        for alias in (False, True):
            part = torch.full((C * P + 64,), SENTINEL, device="cuda")
            zin = z.clone()
            dz = zin if alias else torch.full_like(z, SENTINEL)
            ops.bn_pool_infer_bwd_apply_sums(zin, dpool, am, N, H, W, C, rstd, shift, dz, part)
            torch.cuda.synchronize()
            assert torch.equal(dz, want), "dz differs from ds_bn_pool_infer_bwd_apply (alias=%s)" % alias
            assert bool((part[C * P:] == SENTINEL).all()) and bool((part[:C * P] != SENTINEL).all())
            got = _reduce(part, P, C).astype(np.float64)
            err = np.abs(got - exact)
            bound = 0.0 if integer else (M - 1) * U * np.abs(g).sum(0)
            print("N=%d %dx%d C=%d integer=%s alias=%s: max error %.3e" % (N, H, W, C, integer, alias, err.max()))
            assert (err <= bound).all()
        part2 = torch.full((C * P + 64,), SENTINEL, device="cuda")
        zin = z.clone()
        ops.bn_pool_infer_bwd_apply_sums(zin, dpool, am, N, H, W, C, rstd, shift, None, part2)
        torch.cuda.synchronize()
        assert torch.equal(zin, z) and torch.equal(part2, part)


def test_pooled_stem_form_sums_over_the_pooled_tensors():
    """Only the window maxima of z exist (the stem with MaxPool_2a inside its kernel): dbeta = sum over WINDOWS of
    dpool * [rstd * zmax + shift > 0] -- the pointwise kernel on the pooled tensors without a dz -- equals the sum over pixels
    that the full-resolution twin forms from z, the arg-max record and the same pooled gradient."""
    from tumblr_emotions_amd import ops
    rng = np.random.RandomState(17)
    N, H, W, C = 2, 8, 8, 64
    z = _cuda(np.round(rng.normal(0, 0.3, size=(N, H, W, C)) * 4) / 4)
    rstd = _cuda(2.0 ** rng.randint(-1, 3, size=C))
    shift = _cuda(np.round(rng.normal(0, 0.2, size=C) * 4) / 4)
    OH, OW = H // 2, W // 2
    am = torch.empty(N, OH, OW, C, dtype=torch.uint8, device="cuda")
    y = torch.empty(N, OH, OW, C, device="cuda")
    ops.maxpool_bn_relu_fwd(z, rstd, shift, y, am, N, H, W, C, 3, 2)
    zmax = torch.empty(N, OH, OW, C, device="cuda")
    am2 = torch.empty_like(am)
    ops.maxpool_fwd(z, zmax, am2, N, H, W, C, 3, 2, "SAME")
    dpool = _cuda(rng.randint(-8, 9, size=(N, OH, OW, C)))
    P_full = ops.bn_pool_bwd_partials(N, H, W, C)
    part_full = torch.empty(C * P_full, device="cuda")
    ops.bn_pool_infer_bwd_apply_sums(z, dpool, am, N, H, W, C, rstd, shift, None, part_full)
    Mp = N * OH * OW
    P = ops.bn_infer_bwd_partials(Mp, C)
    part = torch.empty(C * P, device="cuda")
    ops.bn_infer_bwd_apply_sums(zmax, ops.make_segments([(0, C, dpool.data_ptr(), C)]), Mp, C, rstd, shift, None, part)
    a, b = _reduce(part_full, P_full, C), _reduce(part, P, C)
    assert np.array_equal(a, b) and np.abs(a).max() > 0


def test_bad_arguments_return_an_error_and_launch_nothing():
    from tumblr_emotions_amd import ops
    M, C = 8, 16
    z = torch.zeros(M, C, device="cuda")
    dy = torch.ones(M, C, device="cuda")
    rs = torch.ones(C, device="cuda")
    part = torch.full((C * 8,), SENTINEL, device="cuda")
    dz = torch.full((M, C), SENTINEL, device="cuda")
    segs = ops.make_segments([(0, C, dy.data_ptr(), C)])
    bad = [lambda: ops.bn_infer_bwd_apply_sums(z, segs, M, 14, rs, rs, dz, part),                 # C % 4
           lambda: ops.bn_infer_bwd_apply_sums(z, segs, M, C, rs, rs, dz, part, ldz=12),          # ldz < C
           lambda: ops.bn_infer_bwd_apply_sums(z, segs, M, C, rs, rs, dz, None),                  # no partials
           lambda: ops.bn_infer_bwd_apply_sums(z, segs, 0, C, rs, rs, dz, part),                  # M = 0
           lambda: ops.bn_infer_bwd_apply_sums(z, segs, M, C, rs[1:], rs, dz, part),              # misaligned rstd
           lambda: ops.bn_infer_bwd_apply_sums(z, ops.make_segments([(0, 8, dy.data_ptr(), C)]), M, C, rs, rs, dz, part),
           lambda: ops.bn_pool_infer_bwd_apply_sums(z.view(1, 2, 4, C), dy, torch.zeros(1, 1, 2, C, dtype=torch.uint8, device="cuda"),
                                                    1, 2, 4, 14, rs, rs, dz, part),
           lambda: ops.bn_pool_infer_bwd_apply_sums(z.view(1, 2, 4, C), dy, torch.zeros(1, 1, 2, C, dtype=torch.uint8, device="cuda"),
                                                    1, 2, 4, C, rs, rs, dz, None),
           lambda: ops.BnSumJobs([(part, 0, C, dz)]).run(),                                       # P = 0
           lambda: ops.BnSumJobs([(part, 8, 0, dz)]).run()]                                       # C = 0
    for i, call in enumerate(bad):
        with pytest.raises(RuntimeError):
            call()
        torch.cuda.synchronize()
        assert bool((dz == SENTINEL).all()) and bool((part == SENTINEL).all()), i
    assert ops.bn_infer_bwd_partials(0, C) == 0 and ops.bn_infer_bwd_partials(M, 14) == 0


# ---- the step -------------------------------------------------------------------------------------------------------------
DIMS = dict(V=50, D=8, H=64, T=6)
_CACHE = {}


def _inputs(mode, B):
    """Parameters (fp64, random betas), embedding, batch and dropout mask of a step test.  The moving statistics are the fp64
    oracle's BATCH statistics of a different batch, so the activations are O(1) through all 57 layers (with the initialiser's
    (0, 1) the tower's signal vanishes and every comparison is empty)."""
    key = (mode, B)
    if key not in _CACHE:
        rng = np.random.RandomState(101 + B + (mode == "image"))
        if mode == "joint":
            params = R.make_params("joint", rng, num_classes=15, im_features_size=256, embed_dim=DIMS["D"], rnn_size=DIMS["H"],
                                   fc_size=512, dtype=np.float64)
            emb = S.synthetic_embedding(DIMS["V"], DIMS["D"]).astype(np.float64)
        else:
            params = R.make_params("image", rng, num_classes=15, dtype=np.float64)
            emb = None
        for k in params:
            if k.endswith("beta"):
                params[k] = rng.normal(0, 0.1, size=params[k].shape)
        other = S.synthetic_batch(2, DIMS["T"], DIMS["V"], seed=977)
        probe = R.DeepSentimentRef(params, emb, mode, torch.float64)
        with torch.no_grad():
            probe.forward(other)
        assert len(probe.bn_batch_stats) == 57
        for scope, (mean, var) in probe.bn_batch_stats.items():
            params[scope + "/BatchNorm/moving_mean"] = mean.numpy().copy()
            params[scope + "/BatchNorm/moving_variance"] = var.numpy().copy()
        batch = S.synthetic_batch(B, DIMS["T"], DIMS["V"], seed=31 + B)
        mask = (rng.uniform(size=(B, 1024)) < 0.8).astype(np.float64)
        _CACHE[key] = (params, emb, batch, mask)
    return _CACHE[key]


def _net(mode, params, emb, **kw):
    from tumblr_emotions_amd.net import SentimentNet
    kw.setdefault("frozen_bn", True)
    if mode == "joint":
        net = SentimentNet(mode="joint", nb_emotions=15, im_features_size=256, rnn_size=DIMS["H"], fc_size=512, vocab_size=DIMS["V"],
                           embedding_dim=DIMS["D"], post_size=DIMS["T"], **kw)
        net.load_state_dict(dict(params, **{"Text/W_embedding": emb}))
    else:
        net = SentimentNet(mode="image", nb_emotions=15, **kw)
        net.load_state_dict(params)
    return net


def _dev_batch(b):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in b.items()}


# gates of the project's step tests (tests/test_model_gpu.py)
GATE_DECISIONS, GATE_LOGITS, GATE_GRAD, GATE_ADAM = 1e-4, 1e-3, 1e-3, 1e-5


def _step_along_decisions(mode, B):
    """One frozen step against the fp64 reference evaluated along the ReLU masks and pool winners the HIP forward took (the
    protocol of test_model_gpu._joint_step_along_decisions).  Figures are printed before they are asserted."""
    from hip_decisions import hip_decisions, keep_activations
    params, emb, batch, mask = _inputs(mode, B)
    net = _net(mode, params, emb)
    keep_activations(net)
    net.train_step(_dev_batch(batch), 1e-3, dropout_mask=torch.tensor(mask, dtype=torch.float32).cuda())
    torch.cuda.synchronize()
    ref = FrozenBNRef(params, emb, mode, torch.float64)
    ref.inject = hip_decisions(net)
    out = ref.train_step(batch, 1e-3, torch.tensor(mask))
    plain = FrozenBNRef(params, emb, mode, torch.float64).train_step(batch, 1e-3, torch.tensor(mask))
    moved = float((out["logits"] - plain["logits"]).abs().max())
    logits = net.logits.detach().cpu().numpy()
    dlog = np.abs(logits - out["logits"].numpy()).max()
    dloss = abs(net.total_loss_value() - out["loss"])
    print("%s B=%d: decisions move the oracle's logits by %.3e; logits %.3e, loss %.3e (|logits| max %.3f)"
          % (mode, B, moved, dlog, dloss, np.abs(logits).max()))
    grads = net.grads_state_dict()
    n_grads = 71 if mode == "joint" else 65
    assert len(out["grads"]) == n_grads
    rows = []
    for name, g_ref in out["grads"].items():
        g_ref = g_ref.numpy()
        d = grads[name].reshape(g_ref.shape) - g_ref
        rows.append((np.linalg.norm(d) / max(np.linalg.norm(g_ref), 1e-30), np.abs(d).max() / max(np.abs(g_ref).max(), 1e-30), name))
    worst = max(rows)
    print("%s B=%d: worst gradient relative L2 %.3e, max-norm %.3e (%s)" % (mode, B, worst[0], max(r[1] for r in rows), worst[2]))
    after = net.state_dict()
    adam = []
    for name in ref.trainable:
        w_ref = ref.p[name].detach().numpy()
        g_ref = out["grads"][name].numpy()
        big = np.abs(g_ref) > 1e-2 * max(np.abs(g_ref).max(), 1e-12)
        adam.append(((np.abs(after[name].reshape(w_ref.shape) - w_ref)[big] <= GATE_ADAM).mean(), name))
    print("%s B=%d: TF-Adam, smallest share of resolved entries within %.0e: %.4f (%s)" % ((mode, B, GATE_ADAM) + min(adam)))
    assert np.abs(logits).max() > 0.05                      # the tower carries a signal
    assert moved <= GATE_DECISIONS
    assert dlog <= GATE_LOGITS and dloss <= GATE_LOGITS
    for rel, emax, name in rows:
        assert rel <= GATE_GRAD and emax <= GATE_GRAD, "gradient of %s: relative L2 %.3e, max-norm %.3e" % (name, rel, emax)
    for share, name in adam:
        assert share >= 0.99, name
    for name, v in after.items():                            # no UPDATE_OPS in this graph
        if name.endswith(("moving_mean", "moving_variance")):
            assert np.array_equal(v, np.asarray(params[name], np.float32)), name


def test_frozen_joint_step_follows_the_fp64_reference():
    """Joint, B = 4, image tower at 224x224.  The oracle in fp32 against itself in fp64 along the same decisions stays inside
    every gate (scripts/frozen_bn_oracle_spread.py), so the gates are the project's own: decisions 1e-4, logits
    and loss 1e-3, every gradient 1e-3 (relative L2 and max-norm), TF-Adam 1e-5 on the resolved entries."""
    _step_along_decisions("joint", 4)


def test_frozen_image_step_follows_the_fp64_reference():
    _step_along_decisions("image", 2)


def _state(net):
    eng = net.image
    return [net.store.frozen.clone()] + [l.mean.clone() for l in eng.layers]


def test_three_frozen_steps_leave_moving_statistics_and_pivots_bit_identical():
    params, emb, batch, mask = _inputs("joint", 4)
    net = _net("joint", params, emb)
    dev = _dev_batch(batch)
    net.image.alloc(4)                   # (binds the pivots: the moving means)
    before = _state(net)
    theta0 = net.store.theta.clone()
    for _ in range(3):
        net.train_step(dev, 1e-3)
    torch.cuda.synchronize()
    for a, b in zip(before, _state(net)):
        assert torch.equal(a, b)
    assert not torch.equal(theta0, net.store.theta) and bool(torch.isfinite(net.store.theta).all())
    # the same net still evaluates, attributes and visualises as any other
    lg = net.predict(dev, is_training=False).clone()
    lg2, dimg, dwords, _ = net.eval_gradients(dev, 3)
    assert torch.equal(lg, lg2) and bool(torch.isfinite(dimg).all()) and float(dimg.abs().max()) > 0
    assert torch.equal(lg, net.predict(dev, is_training=False, fused=True))
    _, dimg_t = net.input_gradient(dev, 3, seed=5)
    assert bool(torch.isfinite(dimg_t).all())
    net.train_step(dev, 1e-3)
    torch.cuda.synchronize()
    for a, b in zip(before, _state(net)):
        assert torch.equal(a, b)


def test_without_dropout_the_steps_logits_are_predicts_bit_for_bit():
    params, emb, batch, _ = _inputs("joint", 4)
    net = _net("joint", params, emb, dropout_keep_prob=1.0)
    dev = _dev_batch(batch)
    want = net.predict(dev, is_training=False).clone()
    net.train_step(dev, 1e-3)
    torch.cuda.synchronize()
    assert torch.equal(net.logits, want)
    assert not torch.equal(net.predict(dev, is_training=False), want)        # (the step moved the weights)


def test_rows_of_a_frozen_step_are_independent_samples():
    """Replace the images of rows 1-3: row 0 of the step's logits keeps its bits.  On a normal net the batch statistics couple
    the rows, so the same experiment changes row 0."""
    params, emb, batch, mask = _inputs("joint", 4)
    other = dict(batch)
    other["images"] = batch["images"].copy()
    other["images"][1:] = S.synthetic_batch(4, DIMS["T"], DIMS["V"], seed=555)["images"][1:]
    assert np.array_equal(other["images"][0], batch["images"][0]) and not np.array_equal(other["images"][1], batch["images"][1])
    dmask = torch.tensor(mask, dtype=torch.float32).cuda()
    rows = {}
    for frozen in (True, False):
        for name, b in (("a", batch), ("b", other)):
            net = _net("joint", params, emb, frozen_bn=frozen)
            net.train_step(_dev_batch(b), 1e-3, dropout_mask=dmask)
            torch.cuda.synchronize()
            rows[frozen, name] = net.logits.detach().clone()
    assert torch.equal(rows[True, "a"][0], rows[True, "b"][0])
    assert not torch.equal(rows[True, "a"][1:], rows[True, "b"][1:])
    assert not torch.equal(rows[False, "a"][0], rows[False, "b"][0])


def test_no_activation_sized_colsum_in_a_frozen_step_and_zcat_agrees(monkeypatch):
    """Every beta gradient comes out of the pass that writes dz: ds_colsum (counted through its ops wrapper) is only called on
    the [B, .] matrices of the heads and the LSTM's [T * B, 4 H] gates.  And the block-wide pass over a zcat concat gives the per-layer passes' gradients (the
    partial sums are grouped differently: equal up to fp32 summation order, 1e-5 relative L2)."""
    from tumblr_emotions_amd import ops
    params, emb, batch, mask = _inputs("joint", 4)
    dmask = torch.tensor(mask, dtype=torch.float32).cuda()
    calls = []
    real = ops.colsum

    def counting(x, M, C_, ld, scratch, out):
        calls.append((M, C_))
        return real(x, M, C_, ld, scratch, out)

    monkeypatch.setattr(ops, "colsum", counting)
    grads = {}
    for zcat in (True, False):
        net = _net("joint", params, emb)
        net.image.zcat = zcat
        net.train_step(_dev_batch(batch), 1e-3, dropout_mask=dmask)
        torch.cuda.synchronize()
        assert any(st.zcat for st in net.image.stages) == zcat
        grads[zcat] = net.grads_state_dict()
    assert calls, "the wrapper was not reached: the count would be vacuous"
    assert all(M < 4 * 49 for M, _ in calls), calls          # (the smallest activation of the tower is [B * 7 * 7, C])
    worst = max((np.linalg.norm(grads[True][k] - g) / max(np.linalg.norm(g), 1e-30), k) for k, g in grads[False].items())
    print("zcat on / off, worst gradient relative L2: %.3e (%s)" % worst)
    assert worst[0] <= 1e-5


def test_refused_combinations_raise_what_they_say():
    from tumblr_emotions_amd.net import SentimentNet
    from tumblr_emotions_amd.text_model.text_embedding import TextModel
    small = dict(nb_emotions=15, rnn_size=32, vocab_size=50, embedding_dim=8, post_size=6)
    with pytest.raises(NotImplementedError):
        SentimentNet(mode="image", frozen_bn=True, dtype="bf16")
    with pytest.raises(NotImplementedError):
        SentimentNet(mode="image", frozen_bn=True, train_all=True)
    with pytest.raises(ValueError):
        SentimentNet(mode="image", frozen_bn=True, sync_bn=True)
    with pytest.raises(ValueError):
        SentimentNet(mode="text", frozen_bn=True, **small)
    with pytest.raises(ValueError):
        TextModel({"frozen_bn": True, "initial_lr": 1e-3})
    params, emb, batch, _ = _inputs("image", 2)
    net = _net("image", params, emb)
    with pytest.raises(NotImplementedError):
        net.capture_step(_dev_batch(batch))
    assert SentimentNet(mode="text", **small).frozen_bn is False           # off by default


def test_config_key_reaches_the_net_through_the_trainers(tmp_path):
    from tumblr_emotions_amd.image_model.im_model import ImageModel, _CONFIG, train_image_model
    from tumblr_emotions_amd.image_text_model.im_text_rnn_model import train_deep_sentiment
    from tumblr_emotions_amd.text_model.text_embedding import train_text_model
    assert ImageModel(dict(_CONFIG, synthetic=True, frozen_bn=True)).net.frozen_bn is True
    assert ImageModel(dict(_CONFIG, synthetic=True)).net.frozen_bn is False
    small = dict(batch_size=2, num_samples=4, synthetic=True, frozen_bn=True)
    assert np.isfinite(train_image_model(None, str(tmp_path / "image"), 2, config=small, quiet=True))
    joint = dict(small, rnn_size=32, vocab_size=60, embedding_dim=20, post_size=12)
    assert np.isfinite(train_deep_sentiment(None, str(tmp_path / "joint"), 2, config=joint, quiet=True))
    with pytest.raises(ValueError):
        train_text_model(str(tmp_path / "text"), 1, config=joint)


# ---- two ranks --------------------------------------------------------------------------------------------------------------
DP_LR = 1e-3


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _dp_worker(rank, world, port, out):
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    from tumblr_emotions_amd import dp
    dp.init_distributed("gloo", device=0, rank=rank, world_size=world)
    try:
        import torch.distributed as dist
        params, emb, batch, mask = _inputs("joint", 4)
        net = _net("joint", params, emb)
        assert net.world == world and net.reducer.active and net.frozen_bn
        lo, hi = rank * 2, rank * 2 + 2
        local = {k: torch.from_numpy(np.ascontiguousarray(v[lo:hi])).cuda() for k, v in batch.items()}
        net.train_step(local, DP_LR, dropout_mask=torch.tensor(mask[lo:hi], dtype=torch.float32).cuda())
        torch.cuda.synchronize()
        out.put((rank, dict(grads=net.grads_state_dict(), theta=net.store.theta.detach().cpu().numpy(),
                            frozen=net.store.frozen.detach().cpu().numpy())))
    finally:
        dist.destroy_process_group()


def test_two_rank_frozen_step_is_the_single_process_step_on_the_whole_batch():
    """With fixed statistics the samples are independent, so 2 ranks x 2 samples compute what one process computes on the 4
    samples with the concatenated dropout mask: identical weights on both ranks, gradients within 1e-4 relative L2 of the
    single process (fp32 sums taken in another order), weights within 1e-5."""
    import torch.multiprocessing as mp
    from test_dp_gpu import _collect
    ctx = mp.get_context("spawn")
    out = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, out)) for r in range(2)]
    for p in procs:
        p.start()
    got = dict(_collect(out, procs, 2))
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    assert np.array_equal(got[0]["theta"], got[1]["theta"]) and np.isfinite(got[0]["theta"]).all()
    params, emb, batch, mask = _inputs("joint", 4)
    net = _net("joint", params, emb)
    frozen0 = net.store.frozen.detach().cpu().numpy()
    net.train_step(_dev_batch(batch), DP_LR, dropout_mask=torch.tensor(mask, dtype=torch.float32).cuda())
    torch.cuda.synchronize()
    single = net.grads_state_dict()
    worst = (0.0, "")
    for name, g in single.items():
        assert np.array_equal(got[0]["grads"][name], got[1]["grads"][name]), name
        d = got[0]["grads"][name] / 2.0 - g                      # reduced sum / world
        worst = max(worst, (np.linalg.norm(d) / max(np.linalg.norm(g), 1e-30), name))
    dw = np.abs(got[0]["theta"] - net.store.theta.detach().cpu().numpy()).max()
    print("two ranks against one process: worst gradient relative L2 %.3e (%s), weights %.3e" % (worst + (dw,)))
    assert worst[0] <= 1e-4
    assert dw <= 1e-5
    for r in range(2):
        assert np.array_equal(got[r]["frozen"], frozen0)         # moving statistics untouched on every rank
