"""Moving-statistics (is_training=False) gradients on the GPU: the three kernels (ds_bn_infer_bwd_apply,
ds_bn_pool_infer_bwd_apply, ds_token_dot) against NumPy fp64, SentimentNet.eval_gradients against torch.autograd through the
fp64 oracle in evaluation mode, the launches it must not make, the state it must leave alone, integrated_gradients against the
oracle's own midpoint sum, and explain_posts end to end.

Tolerances.  Model level: relative L2 and max-norm <= 1e-3 against the fp64 oracle along the HIP forward's own ReLU / pool
decisions, the gate tests/test_input_grad_gpu.py uses.  Kernel level: see each test."""
import os

import numpy as np
import pytest
import torch

from eval_grad_ref import bn_infer_relu_bwd, maxpool3s2_bwd, token_dot
from oracle import tf_semantics as S
from oracle import torch_ref as R

pytestmark = pytest.mark.gpu

SENTINEL = 12345.678
G = 1024                      # sentinel guard floats on both sides of an output
SMALL_TEXT = dict(batch_size=4, rnn_size=32, vocab_size=60, embedding_dim=20, post_size=12, num_samples=12, synthetic=True)


def _close(got, ref, what, tol):
    d = got - ref
    rel = np.linalg.norm(d) / max(np.linalg.norm(ref), 1e-30)
    emax = np.abs(d).max() / max(np.abs(ref).max(), 1e-30)
    print("%s: relative L2 %.3e, max-norm %.3e" % (what, rel, emax))
    assert rel <= tol and emax <= tol, "%s: relative L2 %.3e, max-norm %.3e" % (what, rel, emax)


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


# ---- the kernels ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("M", [1, 49, 197])
@pytest.mark.parametrize("C_", [4, 20, 64])
def test_bn_infer_bwd_apply_matches_fp64(M, C_):
    """z [M, ldz] with ldz > C, dz written over z between sentinel guards, dy in two segments (one where C = 4: a segment
    boundary is a multiple of four channels).  Seed: 9000 + 100 M + C; z is generated
    from the pre-activation so that no |z*rstd + shift| < 1e-3.  dz against fp64 to 1e-6 relative (the one fp32 rounding, of
    the product, is 6e-8); the mask must be ds_bn_apply_relu's output > 0 exactly."""
    from tumblr_emotions_amd import ops
    rng = np.random.RandomState(9000 + 100 * M + C_)
    ldz = C_ + 4
    rstd = rng.uniform(0.5, 2.0, C_).astype(np.float32)
    shift = rng.normal(0, 0.5, C_).astype(np.float32)
    pre = rng.uniform(0.01, 2.0, (M, C_)) * rng.choice([-1.0, 1.0], (M, C_))
    z = ((pre - shift.astype(np.float64)) / rstd.astype(np.float64)).astype(np.float32)
    assert np.abs(z.astype(np.float64) * rstd + shift).min() >= 1e-3
    total = (rng.uniform(0.1, 1.0, (M, C_)) * rng.choice([-1.0, 1.0], (M, C_))).astype(np.float32)
    cut = 0 if C_ == 4 else (8 if C_ == 20 else 16)          # segment 0 = [0, cut or C), segment 1 the rest
    c0 = cut or C_
    ld0, ld1 = c0 + 8, (C_ - c0) + 4
    seg0 = np.full((M, ld0), np.nan, np.float32); seg0[:, :c0] = total[:, :c0]
    seg1 = np.full((M, max(ld1, 4)), np.nan, np.float32); seg1[:, :C_ - c0] = total[:, c0:]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    s0, s1, r_d, sh_d = dev(seg0), dev(seg1), dev(rstd), dev(shift)
    entries = [(0, c0, s0.data_ptr(), ld0)] + ([(c0, C_, s1.data_ptr(), ld1)] if cut else [])
    segs = ops.make_segments(entries)
    # the forward's decision bits
    y = torch.empty(M, C_, device="cuda")
    ops.bn_apply_relu(dev(z), M, C_, r_d, sh_d, ops.make_segments([(0, C_, y.data_ptr(), C_)]))
    mask = (y > 0).cpu().numpy()
    ref = bn_infer_relu_bwd(z, total.astype(np.float64), rstd, shift)
    assert np.array_equal(ref != 0, mask)
    runs = []
    for _ in range(2):
        host = np.full(G + M * ldz + G, SENTINEL, np.float32)
        host[G:G + M * ldz].reshape(M, ldz)[:, :C_] = z
        buf = dev(host)
        zt = buf[G:G + M * ldz].view(M, ldz)
        ops.bn_infer_bwd_apply(zt, segs, M, C_, r_d, sh_d, zt, ldz=ldz)
        torch.cuda.synchronize()
        out = buf.cpu().numpy()
        assert (out[:G] == np.float32(SENTINEL)).all() and (out[G + M * ldz:] == np.float32(SENTINEL)).all(), "write outside dz"
        body = out[G:G + M * ldz].reshape(M, ldz)
        assert (body[:, C_:] == np.float32(SENTINEL)).all(), "write into the columns past C"
        runs.append(body[:, :C_].copy())
    got = runs[0]
    assert np.array_equal(got != 0, mask), "mask differs from ds_bn_apply_relu's"
    err = np.abs(got - ref)
    assert (err <= 1e-6 * np.abs(ref)).all(), "max relative error %.3e" % (err / np.maximum(np.abs(ref), 1e-30)).max()
    assert np.array_equal(runs[0].view(np.uint32), runs[1].view(np.uint32)), "runs differ"


@pytest.mark.parametrize("H", [9, 8])
def test_bn_pool_infer_bwd_apply_matches_fp64(H):
    """conv -> BN -> ReLU -> 3x3/2 SAME pool, N = 2, C = 8: 9x9 (one row / column of padding on both sides) and 8x8 (the pad
    on the bottom / right edge only).  The pool's arg-max record comes from ds_maxpool_bn_relu_fwd on the same z.  Bound: an
    element of dz is rstd times a sum of up to four pooled gradients, each addition and the product rounded once in fp32:
    1e-6 of rstd * sum |addends| is above 4 * 2^-24 of it.  Seed 9100 + H."""
    from tumblr_emotions_amd import ops
    rng = np.random.RandomState(9100 + H)
    N, W, C_ = 2, H, 8
    OH, OW = (H + 1) // 2, (W + 1) // 2
    rstd = rng.uniform(0.5, 2.0, C_).astype(np.float32)
    shift = rng.normal(0, 0.5, C_).astype(np.float32)
    pre = rng.uniform(0.01, 2.0, (N, H, W, C_)) * rng.choice([-1.0, 1.0], (N, H, W, C_))
    z = ((pre - shift.astype(np.float64)) / rstd.astype(np.float64)).astype(np.float32)
    dpool = rng.standard_normal((N, OH, OW, C_)).astype(np.float32)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    r_d, sh_d, dp_d = dev(rstd), dev(shift), dev(dpool)
    y = torch.empty(N, OH, OW, C_, device="cuda")
    am = torch.empty(N, OH, OW, C_, dtype=torch.uint8, device="cuda")
    ops.maxpool_bn_relu_fwd(dev(z), r_d, sh_d, y, am, N, H, W, C_, 3, 2)
    torch.cuda.synchronize()
    am_h = am.cpu().numpy()
    assert np.array_equal(am_h, S.max_pool_argmax(z, 3, 2, "SAME"))
    g = maxpool3s2_bwd(dpool.astype(np.float64), am_h, H, W)
    gabs = maxpool3s2_bwd(np.abs(dpool).astype(np.float64), am_h, H, W)
    ref = bn_infer_relu_bwd(z, g, rstd, shift)
    assert (ref != 0).any()
    n = N * H * W * C_
    runs = []
    for _ in range(2):
        host = np.full(G + n + G, SENTINEL, np.float32)
        host[G:G + n] = z.ravel()
        buf = dev(host)
        zt = buf[G:G + n].view(N, H, W, C_)
        ops.bn_pool_infer_bwd_apply(zt, dp_d, am, N, H, W, C_, r_d, sh_d, zt)
        torch.cuda.synchronize()
        out = buf.cpu().numpy()
        assert (out[:G] == np.float32(SENTINEL)).all() and (out[G + n:] == np.float32(SENTINEL)).all(), "write outside dz"
        runs.append(out[G:G + n].reshape(N, H, W, C_).copy())
    err = np.abs(runs[0] - ref)
    assert (err <= 1e-6 * rstd * gabs).all(), "max error %.3e" % err.max()
    assert np.array_equal((runs[0] != 0), (ref != 0))
    assert np.array_equal(runs[0].view(np.uint32), runs[1].view(np.uint32)), "runs differ"


@pytest.mark.parametrize("B,T,D", [(1, 1, 1), (3, 7, 20), (5, 12, 300)])
def test_token_dot_matches_fp64(B, T, D):
    """Bound: a D-term fp32 dot product (fused multiply-adds, then a six-step butterfly) is within (D + 8) * 2^-24 of
    sum |terms|.  Rows at t >= seq_len hold NaN inputs and must come out exactly 0.  Seed 9200 + D."""
    from tumblr_emotions_amd import ops
    rng = np.random.RandomState(9200 + D)
    lens = np.array(([1, T, max(1, T // 2), T, 1][:B]), np.int64)
    dx = rng.standard_normal((T * B, D)).astype(np.float32)
    x = rng.standard_normal((T * B, D)).astype(np.float32)
    live = (np.arange(T)[:, None] < lens[None, :]).reshape(T * B)          # row t * B + b
    ref = token_dot(np.where(live[:, None], dx, 0), np.where(live[:, None], x, 0), lens, B, T)
    bound = (D + 8) * 2.0 ** -24 * token_dot(np.abs(np.where(live[:, None], dx, 0)), np.abs(np.where(live[:, None], x, 0)), lens, B, T)
    dx[~live] = np.nan
    x[~live] = np.nan
    dx_d, x_d, l_d = torch.from_numpy(dx).cuda(), torch.from_numpy(x).cuda(), torch.from_numpy(lens).cuda()
    runs = []
    for _ in range(2):
        buf = torch.full((G + B * T + G,), SENTINEL, device="cuda")
        ops.token_dot(dx_d, x_d, l_d, buf[G:G + B * T].view(B, T), B, T, D)
        torch.cuda.synchronize()
        out = buf.cpu().numpy()
        assert (out[:G] == np.float32(SENTINEL)).all() and (out[G + B * T:] == np.float32(SENTINEL)).all(), "write outside out"
        runs.append(out[G:G + B * T].reshape(B, T).copy())
    got = runs[0]
    past = np.arange(T)[None, :] >= lens[:, None]
    assert (got[past].view(np.uint32) == 0).all(), "rows past the length are not exactly +0"
    assert (np.abs(got - ref) <= bound + 1e-45).all(), "max error %.3e" % np.abs(got - ref).max()
    assert np.array_equal(runs[0].view(np.uint32), runs[1].view(np.uint32)), "runs differ"


# ---- the model ------------------------------------------------------------------------------------------------------------

V, D_EMB, HS, T_POST = 40, 12, 16, 7


def _eval_params(mode, rng, batch, emb):
    """Reference-initialised parameters with non-zero beta and NON-TRIVIAL moving statistics: every layer's moving mean /
    variance is that layer's batch statistic on `batch` (one fp32 oracle pass in training mode) perturbed by up to 20 % of a
    standard deviation / 30 %, so evaluation-mode activations keep a realistic spread and every ReLU both passes and blocks."""
    kw = dict(num_classes=15, dtype=np.float64)
    if mode != "image":
        kw.update(embed_dim=D_EMB, rnn_size=HS)
    if mode == "joint":
        kw.update(im_features_size=64, fc_size=48)
    params = R.make_params(mode, rng, **kw)
    for k in params:
        if k.endswith("beta"):
            params[k] = rng.normal(0, 0.1, size=params[k].shape)
    if mode != "text":
        probe = R.DeepSentimentRef(params, emb, mode, torch.float32)
        with torch.no_grad():
            probe.forward(batch, None)
        for scope, (mean, var) in probe.bn_batch_stats.items():
            mean, var = mean.numpy().astype(np.float64), var.numpy().astype(np.float64)
            params[scope + "/BatchNorm/moving_mean"] = mean + rng.uniform(-0.2, 0.2, mean.shape) * np.sqrt(var + 1e-3)
            params[scope + "/BatchNorm/moving_variance"] = var * rng.uniform(0.7, 1.3, var.shape) + 1e-4
    return params


def _distinct_text(B, rng):
    """One distinct table row per (b, t), lengths including 1 and T: the oracle's table gradient, row by row, IS dwords."""
    assert B * T_POST <= V
    texts = np.arange(B * T_POST, dtype=np.int64).reshape(B, T_POST)
    lens = np.array([1, T_POST, 3, 5][:B], np.int64)
    return texts, lens


def _net(mode, params, emb, **kw):
    from tumblr_emotions_amd.net import SentimentNet
    if mode == "image":
        net = SentimentNet(mode="image", nb_emotions=15, **kw)
        net.load_state_dict(params)
    elif mode == "joint":
        net = SentimentNet(mode="joint", nb_emotions=15, im_features_size=64, rnn_size=HS, fc_size=48, vocab_size=V,
                           embedding_dim=D_EMB, post_size=T_POST, **kw)
        net.load_state_dict(dict(params, **{"Text/W_embedding": emb}))
    else:
        net = SentimentNet(mode="text", nb_emotions=15, rnn_size=HS, vocab_size=V, embedding_dim=D_EMB, post_size=T_POST, **kw)
        net.load_state_dict(dict(params, **{"Text/W_embedding": emb}))
    return net


def _dev(batch):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in batch.items()}


def _oracle_gradients(net, ref, batch, target):
    """d(sum target * logits) / d(images) and / d(embedding table) of the fp64 evaluation-mode oracle along the ReLU / pool
    decisions of the HIP forward pass just run (tests/hip_decisions.py; _oracle_dimages of test_input_grad_gpu.py), with the
    un-injected forward as a guard."""
    wrt = []
    feed = dict(batch)
    if ref.mode != "text":
        from hip_decisions import hip_decisions
        ref.inject = None
        with torch.no_grad():
            plain = ref.forward(batch, None).clone()
        ref.inject = hip_decisions(net)
        images = torch.tensor(batch["images"], dtype=torch.float64, requires_grad=True)
        feed["images"] = images
        wrt.append(images)
    if ref.mode != "image":
        wrt.append(ref.embedding)
    logits = ref.forward(feed, None)
    if ref.mode != "text":
        moved = float((logits.detach() - plain).abs().max())
        assert moved <= 1e-4, "following the HIP decisions moved the oracle's logits by %.3e" % moved
    grads = torch.autograd.grad((torch.as_tensor(target, dtype=torch.float64) * logits).sum(), wrt)
    ref.inject = None
    g_im = grads[0].numpy() if ref.mode != "text" else None
    g_emb = grads[-1].numpy() if ref.mode != "image" else None
    return logits.detach().numpy(), g_im, g_emb


def _run_case(mode, B, seed):
    from hip_decisions import keep_activations
    rng = np.random.RandomState(seed)
    batch = S.synthetic_batch(B, T_POST, V, seed=seed, with_images=mode != "text")
    emb = None
    if mode != "image":
        emb = S.synthetic_embedding(V, D_EMB).astype(np.float64)
        batch["texts"], batch["seq_lens"] = _distinct_text(B, rng)
    params = _eval_params(mode, rng, batch, emb)
    target = rng.standard_normal((B, 15)).astype(np.float32)
    net = _net(mode, params, emb)
    if mode != "text":
        assert net.image.stem_pool
        keep_activations(net)
    logits, dimg, dwords, scores = net.eval_gradients(_dev(batch), torch.from_numpy(target).cuda())
    torch.cuda.synchronize()
    ref = R.DeepSentimentRef(params, emb, mode, torch.float64, is_training=False, trainable_embedding=mode != "image")
    ref_logits, g_im, g_emb = _oracle_gradients(net, ref, batch, target)
    assert np.abs(logits.cpu().numpy() - ref_logits).max() <= 1e-3
    if mode == "text":
        assert dimg is None
    else:
        assert tuple(dimg.shape) == (B, 224, 224, 3) and dimg.dtype == torch.float32
        _close(dimg.cpu().numpy().astype(np.float64), g_im, "dimages", 1e-3)
    if mode == "image":
        assert dwords is None and scores is None
        return
    assert tuple(dwords.shape) == (B, T_POST, D_EMB) and tuple(scores.shape) == (B, T_POST)
    ref_dw = g_emb[batch["texts"]]                                   # [B, T, D]: the rows are distinct
    ref_sc = (ref_dw * emb[batch["texts"]]).sum(-1)
    past = np.arange(T_POST)[None, :] >= batch["seq_lens"][:, None]
    assert (ref_dw[past] == 0).all()
    dw, sc = dwords.cpu().numpy(), scores.cpu().numpy()
    assert (dw[past] == 0).all() and (sc[past] == 0).all(), "non-zero past a post's length"
    _close(dw.astype(np.float64), ref_dw, "dwords", 1e-3)
    _close(sc.astype(np.float64), ref_sc, "token_scores", 1e-3)


@pytest.mark.parametrize("B", [1, 3])
def test_eval_gradients_image_mode_matches_autograd(B):
    _run_case("image", B, 70 + B)


def test_eval_gradients_joint_mode_matches_autograd():
    _run_case("joint", 4, 80)


def test_eval_gradients_text_mode_matches_autograd():
    _run_case("text", 3, 90)


def test_eval_gradients_at_batch_32_follows_the_oracle_per_sample():
    """The layout the engine takes at B = 32 -- the default of integrated_gradients: most Mixed blocks leave z in their concat
    (zcat), also in front of a stage pool, and their three closing layers are differentiated by ONE pointwise pass -- against
    the oracle.  Samples are independent under moving statistics, so the fp64 oracle runs on the first and the last sample
    only, along the decisions the HIP forward took for them; those are read from a twin in the materialised layout (zcat off),
    whose four results must be the default layout's bit for bit."""
    from hip_decisions import hip_decisions
    B, pick = 32, [0, 31]
    rng = np.random.RandomState(121)
    batch = S.synthetic_batch(B, T_POST, V, seed=121)
    emb = S.synthetic_embedding(V, D_EMB).astype(np.float64)
    params = _eval_params("joint", rng, {k: v[:4] for k, v in batch.items()}, emb)
    target = rng.standard_normal((B, 15)).astype(np.float32)
    dev, tgt = _dev(batch), torch.from_numpy(target).cuda()
    net = _net("joint", params, emb)
    outs = net.eval_gradients(dev, tgt)
    from tumblr_emotions_amd.engine_image import PoolStage
    zc = [st for st in net.image.stages if getattr(st, "zcat", False)]
    assert len(zc) >= 5 and any(isinstance(getattr(st, "next", None), PoolStage) for st in zc), [st.name for st in zc]
    plain = _net("joint", params, emb)
    plain.image.zcat = False
    ref_outs = plain.eval_gradients(dev, tgt)
    torch.cuda.synchronize()
    for a, b in zip(outs, ref_outs):
        assert np.array_equal(_bits(a), _bits(b)), "zcat and materialised layouts differ at B = 32"
    inj = {k: (v if v is True else np.asarray(v)[pick]) for k, v in hip_decisions(plain).items()}
    sub = {k: v[pick] for k, v in batch.items()}
    sub["texts"] = np.arange(len(pick) * T_POST, dtype=np.int64).reshape(len(pick), T_POST)      # one table row per (b, t)
    table = emb[batch["texts"][pick]].reshape(len(pick) * T_POST, D_EMB)
    ref = R.DeepSentimentRef(params, table, "joint", torch.float64, is_training=False, trainable_embedding=True)
    with torch.no_grad():
        unforced = ref.forward(sub, None).clone()
    ref.inject = inj
    images = torch.tensor(sub["images"], dtype=torch.float64, requires_grad=True)
    logits = ref.forward(dict(sub, images=images), None)
    moved = float((logits.detach() - unforced).abs().max())
    assert moved <= 1e-4, "following the HIP decisions moved the oracle's logits by %.3e" % moved
    g_im, g_emb = torch.autograd.grad((torch.as_tensor(target[pick], dtype=torch.float64) * logits).sum(), [images, ref.embedding])
    assert np.abs(outs[0].cpu().numpy()[pick] - logits.detach().numpy()).max() <= 1e-3
    _close(outs[1].cpu().numpy()[pick].astype(np.float64), g_im.numpy(), "dimages at B = 32", 1e-3)
    ref_dw = g_emb.numpy().reshape(len(pick), T_POST, D_EMB)
    _close(outs[2].cpu().numpy()[pick].astype(np.float64), ref_dw, "dwords at B = 32", 1e-3)
    _close(outs[3].cpu().numpy()[pick].astype(np.float64), (ref_dw * table.reshape(ref_dw.shape)).sum(-1), "token_scores at B = 32", 1e-3)


def _joint_setup(B, seed, **kw):
    rng = np.random.RandomState(seed)
    batch = S.synthetic_batch(B, T_POST, V, seed=seed)
    emb = S.synthetic_embedding(V, D_EMB).astype(np.float64)
    params = _eval_params("joint", rng, batch, emb)
    return _net("joint", params, emb, **kw), _dev(batch), params, emb, batch


def test_eval_gradients_logits_are_predicts_and_targets_agree():
    """Default engine layout (zcat, pooled stem for predict): the logits are predict(is_training=False)'s bit for bit, the
    three target forms give the same bits, a second call repeats the first, and the materialised layout (zcat off) gives
    the same gradient bits as the default one (the block-closing layers differentiated in place inside the concat)."""
    net, dev, params, emb, _ = _joint_setup(2, 101)
    want = net.predict(dev, is_training=False).clone()
    labels = torch.tensor([3, 3], dtype=torch.int64, device="cuda")
    onehot = torch.zeros(2, 15, device="cuda")
    onehot[:, 3] = 1
    outs = [net.eval_gradients(dev, t) for t in (3, labels, onehot, 3)]
    torch.cuda.synchronize()
    assert np.array_equal(_bits(outs[0][0]), _bits(want)), "logits differ from predict(is_training=False)"
    assert np.array_equal(_bits(net.predict(dev, is_training=False)), _bits(want))
    for o in outs[1:]:
        for a, b in zip(outs[0], o):
            assert np.array_equal(_bits(a), _bits(b))
    assert float(outs[0][1].abs().max()) > 0 and float(outs[0][2].abs().max()) > 0
    assert any(getattr(st, "zcat", False) for st in net.image.stages)
    plain = _net("joint", params, emb)
    plain.image.zcat = False
    o = plain.eval_gradients(dev, 3)
    assert not any(getattr(st, "zcat", False) for st in plain.image.stages)
    for a, b in zip(outs[0], o):
        assert np.array_equal(_bits(a), _bits(b)), "zcat and materialised layouts differ"


def test_eval_gradients_launches_no_reduction(monkeypatch):
    """No BatchNorm reduce, finalize or sum-emitting pass during eval_gradients; the pointwise passes cover every BatchNorm
    layer's channels exactly once; no dgrad runs with the DS_EPI_BNSUMS epilogue or the on-load BatchNorm backward."""
    from tumblr_emotions_amd import ops
    net, dev, _, _, _ = _joint_setup(2, 102)
    net.eval_gradients(dev, 1)                      # allocation and weight preparation out of the way
    calls = {}
    covered = []

    def count(name):
        fn = getattr(ops, name)

        def wrapped(*a, **kw):
            calls[name] = calls.get(name, 0) + 1
            return fn(*a, **kw)
        monkeypatch.setattr(ops, name, wrapped)
    banned = ["bn_bwd_reduce", "bn_pool_bwd_reduce", "bn_bwd_finalize", "bn_bwd_finalize_segs", "bn_bwd_finalize_multi",
              "maxpool3_bwd_sums", "bn_bwd_apply", "bn_pool_bwd_apply", "bn_finalize"]
    for name in banned:
        count(name)
    real_apply, real_pool = ops.bn_infer_bwd_apply, ops.bn_pool_infer_bwd_apply
    monkeypatch.setattr(ops, "bn_infer_bwd_apply", lambda z, segs, M, C_, *a, **kw: (covered.append(C_), real_apply(z, segs, M, C_, *a, **kw))[1])
    monkeypatch.setattr(ops, "bn_pool_infer_bwd_apply",
                        lambda z, dp, am, N, H, W, C_, *a, **kw: (covered.append(C_), real_pool(z, dp, am, N, H, W, C_, *a, **kw))[1])
    real_run = ops.LayerPlan.run
    dgrads = []

    def run(self, x, w, z, **kw):
        if self.p.role == ops.DS_CONV_DGRAD:
            dgrads.append((self.d.flags & ops.DS_EPI_BNSUMS, bool(self.d.bnb), kw.get("stats"), kw.get("mask")))
        return real_run(self, x, w, z, **kw)
    monkeypatch.setattr(ops.LayerPlan, "run", run)
    net.eval_gradients(dev, 1)
    torch.cuda.synchronize()
    print("eval_gradients: %d pointwise BatchNorm-backward launches, %d dgrads" % (len(covered), len(dgrads)))
    assert calls == {}, calls
    assert sum(covered) == sum(l.cout for l in net.image.layers) and len(covered) <= len(net.image.layers)
    assert len(dgrads) == len(net.image.layers)
    assert all(d == (0, False, None, None) for d in dgrads), [d for d in dgrads if d != (0, False, None, None)][:3]
    # ... and the training step behind it has its epilogues back
    before = len(dgrads)
    net.input_gradient(dev, 1)
    assert any(d[0] for d in dgrads[before:]), "input_gradient lost its DS_EPI_BNSUMS epilogues"


def test_eval_gradients_leaves_the_training_state_alone():
    """state_dict, Adam m / v and step bit-identical after eval_gradients; predict(fused=True) gives the same bits before and
    after; the next train_steps are bit-identical to those of a twin that never called it (the stem goes back to the pooled
    kernel, the statistics pivots return)."""
    from tumblr_emotions_amd.net import SentimentNet
    rng = np.random.RandomState(62)
    params = R.make_params("image", rng, num_classes=15, dtype=np.float64)
    B = 2
    batch = _dev(S.synthetic_batch(B, 8, 10, seed=4))
    other = _dev(S.synthetic_batch(B, 8, 10, seed=5))
    mask = torch.from_numpy((rng.uniform(size=(B, 1024)) < 0.8).astype(np.float32)).cuda()
    nets = []
    for _ in range(2):
        n = SentimentNet(mode="image", nb_emotions=15)
        n.load_state_dict(params)
        n.train_step(batch, 1e-3, dropout_mask=mask)
        nets.append(n)
    net, twin = nets
    torch.cuda.synchronize()
    st = net.store
    fused_before = net.predict(other, fused=True).clone()
    twin.predict(other, fused=True)
    before = (st.theta.clone(), st.m.clone(), st.v.clone(), net.step, net.state_dict())
    assert net.image.stages[0].layer.pool_inside
    net.eval_gradients(other, 5)
    torch.cuda.synchronize()
    assert not net.image.stages[0].layer.pool_inside
    assert net.image._fused_key is None
    assert torch.equal(st.theta, before[0]) and torch.equal(st.m, before[1]) and torch.equal(st.v, before[2])
    assert net.step == before[3]
    sd = net.state_dict()
    for k, v in before[4].items():
        assert np.array_equal(sd[k], v), k
    fused_after = net.predict(other, fused=True)
    assert np.array_equal(_bits(fused_after), _bits(fused_before))
    twin.predict(other, fused=True)
    for n in (net, twin):
        n.train_step(other, 1e-3, dropout_mask=mask)
        n.train_step(batch, 1e-3, dropout_mask=mask)
    torch.cuda.synchronize()
    assert net.image.stages[0].layer.pool_inside
    assert net.total_loss_value() == twin.total_loss_value()
    assert torch.equal(net.store.theta, twin.store.theta)
    assert torch.equal(net.store.m, twin.store.m) and torch.equal(net.store.v, twin.store.v)
    a, b = net.state_dict(), twin.state_dict()
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def test_eval_gradients_refusals():
    from tumblr_emotions_amd.net import SentimentNet
    rng = np.random.RandomState(61)
    params = R.make_params("image", rng, num_classes=15, dtype=np.float64)
    net = SentimentNet(mode="image", nb_emotions=15)
    net.load_state_dict(params)
    batch = _dev(S.synthetic_batch(2, 8, 10, seed=3))
    with pytest.raises(ValueError):
        net.eval_gradients(batch, torch.zeros(2, 7, device="cuda"))
    with pytest.raises(ValueError):
        net.eval_gradients(batch, torch.tensor([1, 2, 3], device="cuda"))
    with pytest.raises(ValueError):
        net.eval_gradients(batch, 3, text_scale=torch.ones(2))
    with pytest.raises(NotImplementedError):
        net.input_gradient(batch, 3, is_training=False)
    bf = SentimentNet(mode="image", nb_emotions=15, dtype="bf16")
    with pytest.raises(NotImplementedError):
        bf.eval_gradients(batch, 3)
    with pytest.raises(NotImplementedError):
        bf.integrated_gradients(batch, 3)


# ---- integrated gradients -------------------------------------------------------------------------------------------------

def test_integrated_gradients_match_the_oracle_midpoint_sum():
    """steps = 8, joint, B = 2.  The oracle's own 8-midpoint Riemann sum per post: its gradients at the eight interpolated
    inputs (image x0 + alpha (x - x0) with x0 = 0, words alpha * x through a table with one row per (k, t)), along the HIP
    forward's decisions on that very batch of eight.  f_x - f_x0 against two predict calls to 1e-4 absolute.  The
    completeness gap is printed, not gated."""
    from hip_decisions import keep_activations
    steps, B = 8, 2
    rng = np.random.RandomState(111)
    batch = S.synthetic_batch(B, T_POST, V, seed=111)
    batch["seq_lens"] = np.array([3, T_POST], np.int64)
    batch["texts"][0, 3:] = V
    emb = S.synthetic_embedding(V, D_EMB).astype(np.float64)
    params = _eval_params("joint", rng, batch, emb)
    net = _net("joint", params, emb)
    keep_activations(net)
    dev = _dev(batch)
    label = torch.tensor([2, 9], dtype=torch.int64, device="cuda")
    im_attr, tok_attr, delta = net.integrated_gradients(dev, label, steps=steps)
    torch.cuda.synchronize()
    assert tuple(im_attr.shape) == (B, 224, 224, 3) and tuple(tok_attr.shape) == (B, T_POST) and tuple(delta.shape) == (B,)
    alpha = (np.arange(steps) + 0.5) / steps
    onehot = np.zeros((B, 15), np.float32)
    onehot[np.arange(B), label.cpu().numpy()] = 1
    # f_x - f_x0 from two predict calls
    zero = dict(dev, images=torch.zeros_like(dev["images"]), texts=torch.full_like(dev["texts"], V))
    f1 = (net.predict(dev, is_training=False) * torch.from_numpy(onehot).cuda()).sum(1)
    f0 = (net.predict(zero, is_training=False) * torch.from_numpy(onehot).cuda()).sum(1)
    assert float((delta - (f1 - f0)).abs().max()) <= 1e-4
    ref_im, ref_tok = np.zeros((B, 224, 224, 3)), np.zeros((B, T_POST))
    a32 = torch.from_numpy(alpha.astype(np.float32)).cuda()
    for b in range(B):
        x = batch["images"][b].astype(np.float64)
        path = {"images": (a32.view(-1, 1, 1, 1) * dev["images"][b:b + 1]).contiguous(),
                "texts": dev["texts"][b:b + 1].expand(steps, -1).contiguous(),
                "seq_lens": dev["seq_lens"][b:b + 1].expand(steps).contiguous()}
        tgt = np.repeat(onehot[b:b + 1], steps, 0)
        net.eval_gradients(path, torch.from_numpy(tgt).cuda(), text_scale=a32)       # the HIP decisions on this batch of eight
        words = emb[batch["texts"][b]]                                                # [T, D]
        table = (alpha.astype(np.float32).astype(np.float64)[:, None, None] * words[None]).reshape(steps * T_POST, D_EMB)
        ref = R.DeepSentimentRef(params, table, "joint", torch.float64, is_training=False, trainable_embedding=True)
        ob = {"images": path["images"].cpu().numpy(), "texts": np.arange(steps * T_POST, dtype=np.int64).reshape(steps, T_POST),
              "seq_lens": np.repeat(batch["seq_lens"][b:b + 1], steps)}
        _, g_im, g_emb = _oracle_gradients(net, ref, ob, tgt)
        ref_im[b] = x * g_im.mean(0)
        ref_tok[b] = (words * g_emb.reshape(steps, T_POST, D_EMB).mean(0)).sum(-1)
    _close(im_attr.cpu().numpy().astype(np.float64), ref_im, "image attribution", 1e-3)
    _close(tok_attr.cpu().numpy().astype(np.float64), ref_tok, "token attribution", 1e-3)
    total = im_attr.sum(dim=(1, 2, 3)) + tok_attr.sum(dim=1)
    print("completeness gap at %d steps: %s of f_x - f_x0 = %s (oracle sum: %s)" % (
        steps, (total - delta).abs().cpu().numpy(), delta.cpu().numpy(), ref_im.sum(axis=(1, 2, 3)) + ref_tok.sum(axis=1)))


# ---- the front end --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("method", ["gradient", "integrated"])
def test_explain_posts_end_to_end(tmp_path, method):
    from tumblr_emotions_amd.image_text_model import im_text_rnn_model as M
    cfg = dict(SMALL_TEXT)
    ckpt = str(tmp_path / "joint")
    M.train_deep_sentiment(None, ckpt, 2, config=cfg, quiet=True)
    nb, N, T = 2, 2 * cfg["batch_size"], cfg["post_size"]
    res = []
    for name in ("a", "b"):
        out = str(tmp_path / name)
        r = M.explain_posts(ckpt, nb, config=cfg, out_dir=out, method=method, steps=4)
        files = [np.load(os.path.join(out, f + ".npy")) for f in ("saliency_maps", "token_scores", "explained_logits",
                                                                  "explained_post_ids")]
        for a, f in zip(r, files):
            assert np.array_equal(a, f)
        res.append(files)
    maps, tok, logits, ids = res[0]
    assert maps.shape == (N, 224, 224) and tok.shape == (N, T) and logits.shape == (N, 15) and ids.shape == (N,)
    assert np.isfinite(maps).all() and np.isfinite(tok).all() and (maps >= 0).all() and maps.max() > 0 and np.abs(tok).max() > 0
    for a, b in zip(res[0], res[1]):
        assert np.array_equal(a, b), "two runs differ"
    # the saved logits are the ones that were explained: predict(is_training=False) on the same batches, bit for bit, and the
    # saved scores are those of the class they predict (steps == batch_size: the interpolation batches reuse the head's buffers)
    model = M._restored_validation_model(ckpt, cfg)
    bs = cfg["batch_size"]
    for i in range(nb):
        batch = model.next_batch(10 ** 6 + i)
        rows = slice(i * bs, (i + 1) * bs)
        want = model.net.predict(batch, is_training=False).clone()
        assert np.array_equal(logits[rows].view(np.uint32), _bits(want)), "explained_logits are not predict's"
        assert np.array_equal(ids[rows], model.post_ids.cpu().numpy())
        label = want.argmax(dim=1)
        assert np.array_equal(logits[rows].argmax(axis=1), label.cpu().numpy())
        sub = {k: batch[k] for k in ("images", "texts", "seq_lens")}
        if method == "gradient":
            _, dimg, _, sc = model.net.eval_gradients(sub, label)
            attr = dimg * sub["images"]
        else:
            attr, sc, _ = model.net.integrated_gradients(sub, label, steps=4)
        assert np.array_equal(tok[rows].view(np.uint32), _bits(sc)), "token_scores are not those of the predicted class"
        assert np.array_equal(maps[rows].view(np.uint32), _bits(attr.abs().amax(dim=3)))
        lens = batch["seq_lens"].cpu().numpy()
        past = np.arange(T)[None, :] >= lens[:, None]
        assert (tok[rows][past] == 0).all()
    with pytest.raises(ValueError):
        M.explain_posts(ckpt, 1, config=cfg, out_dir=str(tmp_path / "c"), method="lime")
