"""Input gradients on the GPU: the stem's Conv2DBackpropInput kernel (ds_conv_stem_dgrad) against the fp64 adjoint of the
forward conv, SentimentNet.input_gradient against torch.autograd through the oracle, the state it must leave alone, and
class_visualisation (im_text_rnn_model.py:217-339) end to end."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from oracle import tf_semantics as S
from oracle import torch_ref as R

pytestmark = pytest.mark.gpu

SMALL_TEXT = dict(batch_size=8, rnn_size=32, vocab_size=60, embedding_dim=20, post_size=12, num_samples=24,
                  synthetic=True)


def _close(got, ref, what, tol):
    d = got - ref
    rel = np.linalg.norm(d) / max(np.linalg.norm(ref), 1e-30)
    emax = np.abs(d).max() / max(np.abs(ref).max(), 1e-30)
    assert rel <= tol and emax <= tol, "%s: relative L2 %.3e, max-norm %.3e" % (what, rel, emax)


# ---- the kernel ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,H,W,cin", [(2, 32, 32, 4), (3, 37, 29, 3), (5, 64, 64, 4), (1, 224, 224, 4), (4, 224, 224, 3)])
def test_stem_dgrad_matches_the_fp64_adjoint(N, H, W, cin):
    from tumblr_emotions_amd import _lib, ops
    lib = _lib.load()
    rng = np.random.RandomState(N * 1000 + H + W)
    OH, OW = (H + 1) // 2, (W + 1) // 2
    ldx = 64 if N % 2 else 68                         # a padded pixel stride too
    dz = rng.standard_normal((N, OH, OW, ldx)).astype(np.float32)
    w = (rng.standard_normal((7, 7, cin, 64)) * 0.05).astype(np.float32)
    if cin == 4:
        w[:, :, 3, :] = np.nan                         # the zero-padded 4th channel is never read
    ref = S.conv2d_same_bwd_input(dz[..., :64].astype(np.float64), w[:, :, :3, :].astype(np.float64), (N, H, W, 3), 2)
    tol = 2e-4 * np.abs(ref).max()
    dz_d, w_d = torch.from_numpy(dz).cuda(), torch.from_numpy(w).cuda()
    G = 4096                                           # sentinel guards on both sides of dx
    n = N * H * W * 3
    sentinel = 12345.678

    def fresh():
        b = torch.full((G + n + G,), sentinel, device="cuda")
        return b, b[G:G + n]

    plan = ops.LayerPlan(ops.DS_CONV_DGRAD, ops.DS_ARITH_F32, ops.DS_PLAN_PACKED_RGB, N, H, W, cin, 64, 7, 2, ldx, 3, 0)
    assert plan.family == ops.DS_FAM_STEM_DGRAD
    outs = []
    for via in ("plan", "family", "plan"):
        buf, dx = fresh()
        if via == "plan":
            plan.run(ops._p(dz_d), ops._p(w_d), ops._p(dx))
        else:
            assert lib.ds_conv_stem_dgrad(ops._p(dz_d), ops._p(w_d), ops._p(dx), N, H, W, cin, ldx, ops._stream()) == 0
        torch.cuda.synchronize()
        b = buf.cpu().numpy()
        assert (b[:G] == np.float32(sentinel)).all() and (b[G + n:] == np.float32(sentinel)).all(), "write outside dx"
        got = b[G:G + n].reshape(N, H, W, 3)
        assert np.isfinite(got).all()
        err = np.abs(got - ref).max()
        assert err <= tol, "%s: max|dx - ref| = %.3e > %.3e" % (via, err, tol)
        outs.append(got)
    for o in outs[1:]:
        assert np.array_equal(o.view(np.uint32), outs[0].view(np.uint32)), "runs differ"


# ---- the model ----------------------------------------------------------------------------------------------------------

def _oracle_dimages(net, ref, batch, target, mask):
    """d(sum target * logits)/d(images) of the fp64 oracle along the ReLU / pool decisions of the HIP forward pass just run
    (tests/hip_decisions.py, as test_model_gpu._check_step), with the un-injected forward as a guard."""
    from hip_decisions import hip_decisions
    mask_t = None if mask is None else torch.tensor(mask, dtype=torch.float64)
    ref.inject = None
    with torch.no_grad():
        plain = ref.forward(batch, mask_t).clone()
    ref.inject = hip_decisions(net)
    images = torch.tensor(batch["images"], dtype=torch.float64, requires_grad=True)
    logits = ref.forward(dict(batch, images=images), mask_t)
    moved = float((logits.detach() - plain).abs().max())
    assert moved <= 1e-4, "following the HIP decisions moved the oracle's logits by %.3e" % moved
    (g,) = torch.autograd.grad((torch.as_tensor(target, dtype=torch.float64) * logits).sum(), images)
    ref.inject = None
    return logits.detach().numpy(), g.numpy()


def _run_case(mode, B, train_all, with_mask, seed):
    from hip_decisions import keep_activations
    from tumblr_emotions_amd.net import SentimentNet
    rng = np.random.RandomState(seed)
    V, D, Hs, T = 30, 12, 16, 7
    if mode == "image":
        params = R.make_params("image", rng, num_classes=15, dtype=np.float64)
        emb = None
    else:
        params = R.make_params("joint", rng, num_classes=15, im_features_size=64, embed_dim=D, rnn_size=Hs, fc_size=48,
                               dtype=np.float64)
        emb = S.synthetic_embedding(V, D).astype(np.float64)
    for k in params:
        if k.endswith("beta"):
            params[k] = rng.normal(0, 0.1, size=params[k].shape)
    batch = S.synthetic_batch(B, T, V, seed=seed)
    F = 1024
    mask = (rng.uniform(size=(B, F)) < 0.8).astype(np.float32) if with_mask else np.ones((B, F), np.float32)
    target = rng.standard_normal((B, 15)).astype(np.float32)
    if mode == "image":
        net = SentimentNet(mode="image", nb_emotions=15, train_all=train_all)
        net.load_state_dict(params)
    else:
        net = SentimentNet(mode="joint", nb_emotions=15, im_features_size=64, rnn_size=Hs, fc_size=48, vocab_size=V,
                           embedding_dim=D, post_size=T)
        net.load_state_dict(dict(params, **{"Text/W_embedding": emb}))
    assert net.image.stem_pool          # (the default: input_gradient itself moves the stem off the pooled kernel)
    keep_activations(net)
    dev = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in batch.items()}
    logits, dimg = net.input_gradient(dev, torch.from_numpy(target).cuda(), dropout_mask=torch.from_numpy(mask).cuda())
    torch.cuda.synchronize()
    assert tuple(dimg.shape) == (B, 224, 224, 3) and dimg.dtype == torch.float32
    ref = R.DeepSentimentRef(params, emb, mode, torch.float64, train_all=train_all)
    ref_logits, ref_g = _oracle_dimages(net, ref, batch, target, mask)
    assert np.abs(logits.cpu().numpy() - ref_logits).max() <= 1e-3
    _close(dimg.cpu().numpy().astype(np.float64), ref_g, "dimages", 1e-3)


@pytest.mark.parametrize("B,train_all", [(1, False), (2, False), (1, True), (2, True)])
def test_input_gradient_image_mode_matches_autograd(B, train_all):
    _run_case("image", B, train_all, False, 40 + B + 2 * train_all)


@pytest.mark.parametrize("B,with_mask", [(1, False), (4, True)])
def test_input_gradient_joint_mode_matches_autograd(B, with_mask):
    _run_case("joint", B, False, with_mask, 50 + B)


def test_input_gradient_targets_and_refusals():
    from tumblr_emotions_amd.net import SentimentNet
    rng = np.random.RandomState(61)
    params = R.make_params("image", rng, num_classes=15, dtype=np.float64)
    net = SentimentNet(mode="image", nb_emotions=15)
    net.load_state_dict(params)
    batch = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in S.synthetic_batch(2, 8, 10, seed=3).items()}
    ones = torch.ones(2, 1024, device="cuda")
    labels = torch.tensor([3, 3], dtype=torch.int64, device="cuda")
    _, g_int = net.input_gradient(batch, 3, dropout_mask=ones)
    _, g_lab = net.input_gradient(batch, labels, dropout_mask=ones)
    onehot = torch.zeros(2, 15, device="cuda")
    onehot[:, 3] = 1
    _, g_vec = net.input_gradient(batch, onehot, dropout_mask=ones)
    assert torch.equal(g_int, g_lab) and torch.equal(g_int, g_vec)
    with pytest.raises(NotImplementedError):
        net.input_gradient(batch, 3, is_training=False)
    with pytest.raises(ValueError):
        net.input_gradient(batch, torch.zeros(2, 7, device="cuda"))
    text = SentimentNet(mode="text", nb_emotions=15, rnn_size=16, vocab_size=20, embedding_dim=8, post_size=8)
    with pytest.raises(ValueError):
        text.input_gradient(batch, 3)
    bf = SentimentNet(mode="image", nb_emotions=15, dtype="bf16")
    with pytest.raises(NotImplementedError):
        bf.input_gradient(batch, 3)


def test_input_gradient_leaves_the_training_state_alone():
    """state_dict, Adam m / v and step bit-identical after input_gradient; the next train_step bit-identical to that of a
    twin that never computed an input gradient (the stem goes back to the pooled kernel, the statistics pivots return)."""
    from tumblr_emotions_amd.net import SentimentNet
    rng = np.random.RandomState(62)
    params = R.make_params("image", rng, num_classes=15, dtype=np.float64)
    B = 2
    batch = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in S.synthetic_batch(B, 8, 10, seed=4).items()}
    other = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in S.synthetic_batch(B, 8, 10, seed=5).items()}
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
    before = (st.theta.clone(), st.m.clone(), st.v.clone(), net.step, net.state_dict())
    assert net.image.stages[0].layer.pool_inside
    net.input_gradient(other, 5)
    torch.cuda.synchronize()
    assert not net.image.stages[0].layer.pool_inside
    assert torch.equal(st.theta, before[0]) and torch.equal(st.m, before[1]) and torch.equal(st.v, before[2])
    assert net.step == before[3]
    sd = net.state_dict()
    for k, v in before[4].items():
        assert np.array_equal(sd[k], v), k
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


# ---- the front end ------------------------------------------------------------------------------------------------------

def test_class_visualisation_end_to_end(tmp_path):
    from tumblr_emotions_amd.image_text_model import im_text_rnn_model as M
    from tumblr_emotions_amd.preprocessing.inception_preprocessing import preprocess_image
    cfg = dict(SMALL_TEXT, batch_size=4, num_samples=12)
    ckpt = str(tmp_path / "joint")
    M.train_deep_sentiment(None, ckpt, 2, config=cfg, quiet=True)
    label, lr, seed = 3, 150.0, 7
    out1, out2 = str(tmp_path / "a"), str(tmp_path / "b")
    img1 = M.class_visualisation(label, lr, ckpt, config=cfg, num_iterations=20, seed=seed, out_dir=out1)
    img2 = M.class_visualisation(label, lr, ckpt, config=cfg, num_iterations=20, seed=seed, out_dir=out2)
    assert img1.shape == (224, 224, 3) and np.isfinite(img1).all()
    assert np.array_equal(img1, img2)
    saved = np.load(os.path.join(out1, "class_visualisation_%d.npy" % label))
    assert np.array_equal(saved, img1)
    start = preprocess_image(np.random.RandomState(seed).standard_normal((224, 224, 3)).astype(np.float32), 224, 224)
    assert not np.array_equal(start, img1)
    model = M._restored_validation_model(ckpt, cfg)
    net = model.net
    post = net.text.T
    batch = {"texts": torch.full((1, post), net.text.V - 1, dtype=torch.int64, device="cuda"),
             "seq_lens": torch.full((1,), post, dtype=torch.int64, device="cuda")}
    ones = torch.ones(1, 1024, device="cuda")
    score = []
    for im in (start, img1):
        batch["images"] = torch.from_numpy(np.ascontiguousarray(im[None])).cuda()
        logits, _ = net.input_gradient(batch, label, dropout_mask=ones)
        score.append(float(logits[0, label]))
    assert score[1] > score[0], score
