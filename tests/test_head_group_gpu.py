"""The grouped head chain (JointHeadEngine.group / InceptionV1Engine.head_group, default on): W_fc's two halves as one
ds_gemm_group + ds_slab_epilogue_group launch pair, both feature gradients as one GEMM through W_fc with two outputs, the cross
entropy in the W_softmax combine (ds_slab_epilogue_ce, eager and captured step), the parameter gradients off the chain.  Every result
keeps the bits of the separate launches; each is also held against an fp64 NumPy evaluation of its own inputs at the kernel
tests' bound, 2e-4 * max|ref|."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

IM, TX, FC, NC = 256, 512, 512, 15      # the joint model's own head
LD_IM, LD_TX = IM + 8, TX + 4           # the engines hand over features whose row stride exceeds their width
BATCHES = (3, 33, 130)                  # a partial 32-row block; one row past a block; the second 128-row tile
REL = 2e-4


def _close(got, ref, what):
    ref = np.asarray(ref, np.float64)
    err = float(np.abs(got.detach().cpu().numpy().astype(np.float64) - ref).max())
    bound = REL * float(np.abs(ref).max())
    print("%s: max|err| = %.3e, bound %.3e" % (what, err, bound))
    assert err <= bound, (what, err, bound)


def _f64(t):
    return t.detach().cpu().numpy().astype(np.float64)


@pytest.fixture(scope="module")
def head():
    """Operands shared by the kernel-level tests (never written by them): per batch size the two strided feature tensors and
    labels; one set of weights."""
    g = torch.Generator().manual_seed(11)
    w = {"W_fc": torch.randn(IM + TX, FC, generator=g) * 0.05, "b_fc": torch.randn(FC, generator=g) * 0.1,
         "W_sm": torch.randn(FC, NC, generator=g) * 0.1, "b_sm": torch.randn(NC, generator=g) * 0.1}
    w = {k: v.cuda() for k, v in w.items()}
    per = {}
    for B in BATCHES:
        im = torch.randn(B, LD_IM, generator=g).cuda()[:, :IM]
        tx = torch.randn(B, LD_TX, generator=g).cuda()[:, :TX]
        per[B] = (im, tx, torch.randint(0, NC, (B,), generator=g).cuda())
    return w, per


def _plans(B):
    from tumblr_emotions_amd import ops
    from tumblr_emotions_amd.ops import DS_EPI_ACCUM, DS_EPI_BIAS, DS_EPI_RELU, head_gemm_plan
    dev = torch.device("cuda")
    fc_im = head_gemm_plan(B, IM, FC, LD_IM, FC, FC, device=dev)
    fc_tx = head_gemm_plan(B, TX, FC, LD_TX, FC, FC, flags=DS_EPI_ACCUM | DS_EPI_BIAS | DS_EPI_RELU, device=dev)
    assert isinstance(fc_im, ops.SplitGemm) and isinstance(fc_tx, ops.SplitGemm) and (fc_im.splits, fc_tx.splits) == (4, 8)
    return fc_im, fc_tx


def _dense_reference(B, w, im, tx):
    """Today's sequence: fc_im (plain), then fc_tx with ACCUM | BIAS | RELU."""
    from tumblr_emotions_amd import ops
    fc_im, fc_tx = _plans(B)
    dense = torch.empty(B, FC, device="cuda")
    w_im, w_tx = C.c_void_p(w["W_fc"].data_ptr()), C.c_void_p(w["W_fc"].data_ptr() + 4 * IM * FC)
    fc_im.run(ops._p(im), w_im, ops._p(dense))
    fc_tx.run(ops._p(tx), w_tx, ops._p(dense), bias=ops._p(w["b_fc"]))
    return dense, fc_im.slabs, fc_tx.slabs


@pytest.mark.parametrize("B", BATCHES)
def test_dense_two_problems_one_output(head, B):
    """group{fc_im, fc_tx} -> dense = relu(sum slabs_tx + b_fc + sum slabs_im): slabs and dense bit for bit, three calls in a
    row on the same buffers."""
    from tumblr_emotions_amd import ops
    from tumblr_emotions_amd.ops import DS_EPI_ACCUM, DS_EPI_BIAS, DS_EPI_RELU
    w, per = head
    im, tx, _ = per[B]
    ref, slabs_im, slabs_tx = _dense_reference(B, w, im, tx)
    fc_im, fc_tx = _plans(B)
    dense = torch.full((B, FC), float("nan"), device="cuda")
    grp = ops.GemmGroup([fc_im, fc_tx], [ops.slab_combine(fc_tx, dense.data_ptr(), FC, flags=DS_EPI_ACCUM | DS_EPI_BIAS | DS_EPI_RELU,
                                                          bias=w["b_fc"].data_ptr(), pre=fc_im)])
    w_im, w_tx = C.c_void_p(w["W_fc"].data_ptr()), C.c_void_p(w["W_fc"].data_ptr() + 4 * IM * FC)
    for _ in range(3):
        grp.run((ops._p(im), ops._p(tx)), (w_im, w_tx))
        assert torch.equal(fc_im.slabs, slabs_im) and torch.equal(fc_tx.slabs, slabs_tx)
        assert torch.equal(dense, ref)
    W = _f64(w["W_fc"])
    _close(dense, np.maximum(_f64(im) @ W[:IM] + _f64(tx) @ W[IM:] + _f64(w["b_fc"]), 0.0), "dense B=%d" % B)


@pytest.mark.parametrize("B", BATCHES)
def test_logits_and_cross_entropy_in_one_combine(head, B):
    """The W_softmax GEMM's combine going on to loss and dlogits: the bits of ds_slab_epilogue + ds_softmax_ce."""
    from tumblr_emotions_amd import ops
    from tumblr_emotions_amd.ops import DS_EPI_BIAS, head_gemm_plan
    w, per = head
    im, tx, labels = per[B]
    dense = _dense_reference(B, w, im, tx)[0]
    dev = torch.device("cuda")
    sm = head_gemm_plan(B, FC, NC, FC, NC, NC, flags=DS_EPI_BIAS, device=dev)
    assert isinstance(sm, ops.SplitGemm)
    logits_ref, loss_ref, dl_ref = torch.empty(B, NC, device=dev), torch.zeros(1, device=dev), torch.empty(B, NC, device=dev)
    sm.run(ops._p(dense), ops._p(w["W_sm"]), ops._p(logits_ref), bias=ops._p(w["b_sm"]))
    ops.softmax_ce(logits_ref, labels, B, NC, 1.0, None, loss_ref, dl_ref)
    sm2 = head_gemm_plan(B, FC, NC, FC, NC, NC, flags=DS_EPI_BIAS, device=dev)
    logits, loss, dl = (torch.full((B, NC), float("nan"), device=dev), torch.full((1,), float("nan"), device=dev),
                        torch.full((B, NC), float("nan"), device=dev))
    for _ in range(3):
        ops.split_gemm_ce(sm2, ops._p(dense), ops._p(w["W_sm"]), logits, ops._p(w["b_sm"]), labels, loss, dl)
        assert torch.equal(sm2.slabs, sm.slabs)
        assert torch.equal(logits, logits_ref) and torch.equal(loss, loss_ref) and torch.equal(dl, dl_ref)
    z = _f64(dense) @ _f64(w["W_sm"]) + _f64(w["b_sm"])
    _close(logits, z, "logits B=%d" % B)
    z = _f64(logits)
    m = z.max(1, keepdims=True)
    e = np.exp(z - m)
    s = e.sum(1, keepdims=True)
    y = labels.cpu().numpy()
    _close(loss, [np.mean(m[:, 0] + np.log(s[:, 0]) - z[np.arange(B), y])], "loss B=%d" % B)
    onehot = np.zeros((B, NC))
    onehot[np.arange(B), y] = 1.0
    _close(dl, (e / s - onehot) / B, "dlogits B=%d" % B)


@pytest.mark.parametrize("B", BATCHES)
def test_feature_gradients_one_problem_two_outputs(head, B):
    """ddense W_fc^T as ONE GEMM over W_fc's im + tx rows, columns [0, im) -> d_im, [im, im + tx) -> d_tx: the bits of the
    im_dgrad and tx_dgrad launches."""
    from tumblr_emotions_amd import ops
    from tumblr_emotions_amd.ops import head_gemm_plan
    w, per = head
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(100 + B)
    dd = (torch.randn(B, FC, generator=g) * (torch.rand(B, FC, generator=g) > 0.5)).cuda()
    w_im, w_tx = C.c_void_p(w["W_fc"].data_ptr()), C.c_void_p(w["W_fc"].data_ptr() + 4 * IM * FC)
    im_dgrad = head_gemm_plan(B, FC, IM, FC, IM, FC, transposed_w=True, device=dev)
    tx_dgrad = head_gemm_plan(B, FC, TX, FC, TX, FC, transposed_w=True, device=dev)
    d_im_ref, d_tx_ref = torch.empty(B, IM, device=dev), torch.empty(B, TX, device=dev)
    im_dgrad.run(ops._p(dd), w_im, ops._p(d_im_ref))
    tx_dgrad.run(ops._p(dd), w_tx, ops._p(d_tx_ref))
    fc_dgrad = head_gemm_plan(B, FC, IM + TX, FC, IM + TX, FC, transposed_w=True, device=dev)
    assert isinstance(fc_dgrad, ops.SplitGemm) and fc_dgrad.splits == im_dgrad.splits == tx_dgrad.splits
    d_im, d_tx = torch.full((B, IM), float("nan"), device=dev), torch.full((B, TX), float("nan"), device=dev)
    grp = ops.GemmGroup([fc_dgrad], [ops.slab_combine(fc_dgrad, d_im.data_ptr(), IM, out2=d_tx.data_ptr(), ldo2=TX, n_split=IM)])
    for _ in range(3):
        grp.run((ops._p(dd),), (w_im,))
        assert torch.equal(fc_dgrad.slabs[:, :, :IM], im_dgrad.slabs) and torch.equal(fc_dgrad.slabs[:, :, IM:], tx_dgrad.slabs)
        assert torch.equal(d_im, d_im_ref) and torch.equal(d_tx, d_tx_ref)
    full = _f64(dd) @ _f64(w["W_fc"]).T
    _close(d_im, full[:, :IM], "d_im B=%d" % B)
    _close(d_tx, full[:, IM:], "d_tx B=%d" % B)


@pytest.mark.parametrize("B", BATCHES)
def test_gemm_group_of_four_kernel_variants(head, B):
    """One ds_gemm_group launch over four problems that need the four instantiations of the small-tile kernel (weights n- or
    k-contiguous, 16-byte or scalar loads; split-K or not): every output is what the problem's own ds_conv_igemm launch writes."""
    from tumblr_emotions_amd import _lib, ops
    from tumblr_emotions_amd.ops import gemm_plan
    w, per = head
    im, tx, _ = per[B]
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(200 + B)
    dense = torch.randn(B, FC, generator=g).cuda()
    dl = torch.randn(B, NC, generator=g).cuda()
    w_tx = C.c_void_p(w["W_fc"].data_ptr() + 4 * IM * FC)
    problems = [      # (plan, x, w, output floats)
        (gemm_plan(B, IM, FC, LD_IM, FC, FC, splits=4, z_split_stride=B * FC), im, ops._p(w["W_fc"]), 4 * B * FC),
        (gemm_plan(B, FC, NC, FC, NC, NC, splits=8, z_split_stride=B * NC), dense, ops._p(w["W_sm"]), 8 * B * NC),
        (gemm_plan(B, FC, TX, FC, TX, FC, transposed_w=True, splits=8, z_split_stride=B * TX), dense, w_tx, 8 * B * TX),
        (gemm_plan(B, NC, FC, NC, FC, NC, transposed_w=True), dl, ops._p(w["W_sm"]), B * FC)]
    lib = _lib.load()
    refs, outs = [], []
    for plan, x, wp, n in problems:
        z = torch.full((n,), float("nan"), device=dev)
        _lib.check(lib.ds_conv_igemm(C.byref(plan.d), ops._p(x), wp, ops._p(z), None, None, None, None, ops._stream()), "ds_conv_igemm")
        refs.append(z)
        outs.append(torch.full((n,), float("nan"), device=dev))
    n = len(problems)
    descs = (C.POINTER(_lib.ConvDesc) * n)(*[C.pointer(p[0].d) for p in problems])
    xs = (C.c_void_p * n)(*[p[1].data_ptr() for p in problems])
    ws = (C.c_void_p * n)(*[p[2].value for p in problems])
    zs = (C.c_void_p * n)(*[o.data_ptr() for o in outs])
    for _ in range(3):
        _lib.check(lib.ds_gemm_group(descs, xs, ws, zs, n, ops._stream()), "ds_gemm_group")
        for i, (o, r) in enumerate(zip(outs, refs)):
            assert not bool(torch.isnan(o).any()) and torch.equal(o, r), "problem %d" % i
    _close(outs[3].view(B, FC), _f64(dl) @ _f64(w["W_sm"]).T, "sm_dgrad-shaped problem B=%d" % B)
    _close(outs[1].view(8, B, NC).sum(0), _f64(dense) @ _f64(w["W_sm"]), "W_softmax slabs B=%d" % B)
    # a fifth problem, or one that is not a plain GEMM without epilogue, is refused before anything is launched
    assert lib.ds_gemm_group(descs, xs, ws, zs, 5, ops._stream()) == -1
    bad = gemm_plan(B, IM, FC, LD_IM, FC, FC, flags=ops.DS_EPI_RELU)
    descs1 = (C.POINTER(_lib.ConvDesc) * 1)(C.pointer(bad.d))
    assert lib.ds_gemm_group(descs1, xs, ws, zs, 1, ops._stream()) == -1 and b"ds_gemm_group" in lib.ds_last_error()


# ---- step level -------------------------------------------------------------------------------------------------------------

def _run_steps(mode, on, monkeypatch, captured=False):
    from tumblr_emotions_amd import _lib
    from tumblr_emotions_amd.net import SentimentNet
    from tumblr_emotions_amd.synthetic import synthetic_batch_numpy, to_device
    batch = to_device(synthetic_batch_numpy(8, 10, 50, seed=5))
    net = SentimentNet(mode=mode, nb_emotions=NC, im_features_size=IM, rnn_size=TX, fc_size=FC, vocab_size=50, embedding_dim=20,
                       post_size=10)
    if net.head is not None:
        net.head.group = on
    net.image.head_group = on
    net.initialize(seed=7)
    calls, every = [], []
    check = _lib.check
    monkeypatch.setattr(_lib, "check", lambda rc, what: (calls.append(what), every.append(what), check(rc, what))[2])
    if captured:
        assert net.capture_step(batch)
    net.train_step(batch, 1e-3)
    g1 = net.store.grad.clone()
    del calls[:]
    net.train_step(batch, 1e-3)
    torch.cuda.synchronize()
    monkeypatch.setattr(_lib, "check", check)
    return calls, every, (net.logits.clone(), net.total_loss_value(), g1, net.store.grad.clone(), net.store.theta.clone(),
                   net.store.frozen.clone())


def _same(a, b):
    for x, y in zip(a, b):
        if torch.is_tensor(x):
            assert not bool(torch.isnan(x).any())
            assert torch.equal(x, y)
        else:
            assert x == x and x == y


def test_joint_step_is_bit_identical(monkeypatch):
    """Two joint training steps at batch 8 with the model's own head dims, switch on and off: logits, loss, every gradient, the
    updated parameters and the BatchNorm moving statistics are BIT-identical -- and the launches really differ."""
    on_calls, on_every, on = _run_steps("joint", True, monkeypatch)
    off_calls, off_every, off = _run_steps("joint", False, monkeypatch)
    # the step-level anchor of the fused cross entropy: on forms it in the W_softmax combine, off with ds_softmax_ce
    assert "ds_slab_epilogue_ce" in on_every and "ds_softmax_ce" in off_every and "ds_slab_epilogue_ce" not in off_every
    assert on_calls.count("ds_gemm_group") == 1 and on_calls.count("ds_slab_epilogue_group") == 2
    assert "ds_gemm_group" not in off_calls and "ds_slab_epilogue_group" not in off_calls
    # the Logits layer: input gradient and the pool's gradient first, then the leaves
    i = on_calls.index("ds_avgpool_dropout_bwd")
    assert on_calls[i + 1] == "ds_conv_wgrad" and off_calls[off_calls.index("ds_avgpool_dropout_bwd") + 1] != "ds_conv_wgrad"
    assert len(on_calls) < len(off_calls)
    _same(on, off)


def test_image_step_is_bit_identical(monkeypatch):
    """The same in mode="image": the Logits layer's weight and bias gradient (and the L2 term) leave the chain."""
    on_calls, _, on = _run_steps("image", True, monkeypatch)
    off_calls, _, off = _run_steps("image", False, monkeypatch)
    i = on_calls.index("ds_avgpool_dropout_bwd")
    assert on_calls[i + 1:i + 4] == ["ds_conv_wgrad", "ds_colsum", "ds_sumsq"]
    assert off_calls[off_calls.index("ds_avgpool_dropout_bwd") + 1] != "ds_conv_wgrad"
    assert sorted(on_calls) == sorted(off_calls)
    _same(on, off)


def test_captured_step_equals_the_eager_step(monkeypatch):
    """Switch on: a captured joint step (one side stream in the capture) replayed twice leaves the bits of two eager steps; both
    form the cross entropy in the W_softmax combine (against ds_softmax_ce: test_joint_step_is_bit_identical)."""
    _, eager_all, eager = _run_steps("joint", True, monkeypatch)
    cap_calls, cap_all, cap = _run_steps("joint", True, monkeypatch, captured=True)
    assert "ds_slab_epilogue_ce" in eager_all and "ds_slab_epilogue_ce" in cap_all and "ds_gemm_group" in cap_all
    assert cap_calls == []      # (a replay launches the graph, nothing else)
    _same(eager, cap)
