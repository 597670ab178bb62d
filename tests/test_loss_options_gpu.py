"""label_smoothing and class_weights on the GPU: ds_softmax_ce_opts and ds_slab_epilogue_ce_opts against fp64
of the same fp32 logits (tests/loss_ref.py) and against the existing entry points (bit for bit at the defaults), then the
training step in its three modes, with clones, two ranks and a captured step, and the text front end.  [TF-sem]: TF's
softmax_cross_entropy(weights, label_smoothing) restated, parity unpinned.

Kernel tolerances are rounding counts derived in loss_ref.row_floor / loss_ref.check_ce; none was measured.  Each kernel test
prints its worst error / bound ratio.  On an MI355X: ds_softmax_ce_opts <= 0.103 (dlogits per row; the loss <= 0.028),
ds_slab_epilogue_ce_opts <= 0.096; the file takes about 10 s."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import head_ref as HR
import loss_ref as LR
from oracle import tf_semantics as S
from oracle import torch_ref as R
from test_dp_gpu import TEXT, _collect, _free_port
from test_ema_gpu import _batch, _bits, _net
from test_frontends_gpu import SMALL_TEXT
from hip_decisions import keep_activations
from test_model_gpu import _check_step, _grad_close, _sync_from_oracle

pytestmark = pytest.mark.gpu

NAN = float("nan")
GUARD = 7.0
EPSILONS = (0.0, 0.1, 0.9)
# per-class weights of the step tests: non-uniform, one zero
CW15 = [0.5, 2.0, 0.0, 1.0, 1.5, 0.25, 3.0, 1.0, 0.75, 1.25, 2.5, 0.1, 1.0, 4.0, 0.6]
KEYS = dict(label_smoothing=0.1, class_weights=CW15)


def _ops():
    from tumblr_emotions_amd import ops
    return ops


def dev(a, dtype=torch.float32):
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda")


def host(t):
    return t.detach().cpu().numpy().copy()


def _weight_settings(rng, C_, y):
    """NULL, all ones, some zeros (P < B: the class of row 0 is dead; another drawn class stays alive wherever two classes
    are drawn), and zeros on every drawn class (P == 0)."""
    some = rng.uniform(0.25, 2.0, size=C_).astype(np.float32)
    some[np.arange(C_) % 4 == 1] = 0.0
    some[y[0]] = 0.0
    others = [c for c in np.unique(y) if c != y[0]]
    if others:
        some[others[0]] = 1.5
    none = rng.uniform(0.25, 2.0, size=C_).astype(np.float32)
    none[np.unique(y)] = 0.0
    return (("null", None), ("ones", np.ones(C_, np.float32)), ("zeros", some), ("dead", none))


def _run_ce(ops, zd, yd, B, C_, eps, cwd, up, loss, dl):
    ops.softmax_ce_opts(ops.ce_desc(eps, cwd), zd, yd, B, C_, 1.5, up, loss, dl)


# ---- ds_softmax_ce_opts --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B", [1, 255, 256, 257, 513])
def test_softmax_ce_opts_rows_classes_smoothing_weights_and_poisoned_labels(B):
    """The grid of test_softmax_ce_rows_classes_and_poisoned_labels (one workgroup; B crosses one and two trips; logits uniform
    over +-60, one row of equal logits, the upstream scale on the device: 1.5 from the host x 0.5) times label_smoothing in
    0, 0.1, 0.9 times four weight vectors (_weight_settings).  Against fp64 of the fp32 inputs: the loss within 1e-5 of |ref|;
    dlogits per row within 1e-5 of the row's max|ref| + (C + 9) u w_b k, k = grad_scale / P (loss_ref.row_floor derives it: the
    C + 7 roundings of HR.ce_row_floor, one more for q and one for w, scaled by the row's own factor; a row of weight 0 must
    be exactly 0).  P == 0: loss 0.0 and all dlogits 0.0.  Guard words behind both outputs stay; with either output NULL the
    other keeps its bits; all-ones weights give the bits of NULL weights; {0, NULL} gives ds_softmax_ce's bits.  A label of C
    or -1 in a counted row: the loss is NaN, that row is finite and follows the formula with w = 1, every other row keeps
    its bits."""
    ops = _ops()
    worst = HR.Worst()
    up = dev([0.5])
    gs = 1.5 * 0.5
    for C_ in (1, 2, 15, 32, 33):
        rng = np.random.RandomState(B + 13 * C_)
        for equal_row in ([None, 0] if B == 1 else [B // 2]):
            z = rng.uniform(-60, 60, size=(B, C_)).astype(np.float32)
            if equal_row is not None:
                z[equal_row] = z[equal_row, 0]
            y = rng.randint(0, C_, size=B)
            zd, yd = dev(z), dev(y, torch.int64)
            plain_loss, plain_dl = torch.full((1,), NAN, device="cuda"), torch.full((B, C_), NAN, device="cuda")
            ops.softmax_ce(zd, yd, B, C_, 1.5, up, plain_loss, plain_dl)
            for eps in EPSILONS:
                null_bits = None
                for name, cw in _weight_settings(np.random.RandomState(7 * B + C_), C_, y):
                    cwd = None if cw is None else dev(cw)
                    what = "ds_softmax_ce_opts B=%d C=%d eps=%g weights=%s" % (B, C_, eps, name)
                    loss, dl = torch.full((2,), GUARD, device="cuda"), torch.full((B * C_ + 4,), GUARD, device="cuda")
                    _run_ce(ops, zd, yd, B, C_, eps, cwd, up, loss, dl)
                    loss_only, dl_only = torch.full((1,), NAN, device="cuda"), torch.full((B * C_,), NAN, device="cuda")
                    _run_ce(ops, zd, yd, B, C_, eps, cwd, up, loss_only, None)
                    _run_ce(ops, zd, yd, B, C_, eps, cwd, up, None, dl_only)
                    torch.cuda.synchronize()
                    assert host(loss)[1] == GUARD and (host(dl)[B * C_:] == GUARD).all(), what + ": wrote past its outputs"
                    got_loss, got_dl = host(loss)[:1], host(dl)[:B * C_].reshape(B, C_)
                    HR.check_bits(host(loss_only), got_loss, what + " loss alone")
                    HR.check_bits(host(dl_only).reshape(B, C_), got_dl, what + " dlogits alone")
                    LR.check_ce(got_loss, got_dl, z, y, eps, cw, gs, what, worst)
                    w = np.ones(B) if cw is None else cw[y].astype(np.float64)
                    P = int((w != 0).sum())
                    if name == "zeros":
                        assert P < B and (P > 0 or len(np.unique(y)) == 1), what
                        HR.check_bits(got_dl[w == 0], np.zeros_like(got_dl[w == 0]), what + " rows of weight 0")
                    if name == "dead":
                        assert P == 0, what
                        HR.check_bits(got_loss, np.zeros(1, np.float32), what + " loss with no counted row")
                        HR.check_bits(got_dl, np.zeros_like(got_dl), what + " dlogits with no counted row")
                    if name == "null":
                        null_bits = (got_loss, got_dl)
                        if eps == 0.0:
                            HR.check_bits(got_loss, host(plain_loss), what + " against ds_softmax_ce")
                            HR.check_bits(got_dl, host(plain_dl), what + " against ds_softmax_ce")
                    if name == "ones":
                        HR.check_bits(got_loss, null_bits[0], what + " against NULL weights")
                        HR.check_bits(got_dl, null_bits[1], what + " against NULL weights")
                    # a label outside [0, C), in a row that counts (so that P, and with it every other row, stays)
                    counted = np.flatnonzero(w != 0)
                    r = int(counted[len(counted) // 3]) if len(counted) else B // 3
                    for bad_label in (C_, -1):
                        yb = y.copy()
                        yb[r] = bad_label
                        loss_b, dl_b = torch.full((1,), 0.0, device="cuda"), torch.full((B, C_), NAN, device="cuda")
                        _run_ce(ops, zd, dev(yb, torch.int64), B, C_, eps, cwd, up, loss_b, dl_b)
                        torch.cuda.synchronize()
                        got_b = host(dl_b)
                        LR.check_ce(host(loss_b), got_b, z, yb, eps, cw, gs, what + " label %d" % bad_label, worst)
                        assert np.isnan(host(loss_b)[0]), what + ": label %d did not poison the loss" % bad_label
                        if len(counted):
                            rest = np.arange(B) != r
                            HR.check_bits(got_b[rest], got_dl[rest], what + " rows beside the poisoned one")
    print("ds_softmax_ce_opts B=%d: %s" % (B, worst))


# ---- ds_slab_epilogue_ce_opts ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("M", [1, 256, 257, 512])
def test_slab_epilogue_ce_opts_is_the_combine_followed_by_softmax_ce_opts(M):
    """Eight slabs + bias -> logits -> loss, dlogits in one workgroup: the bits of ds_slab_epilogue(DS_EPI_BIAS) followed by
    ds_softmax_ce_opts, for N in 1, 15, 32, smoothing 0.1 and weights with zeros; with a {0, NULL} descriptor (and with none)
    the bits of ds_slab_epilogue_ce.  The loss and dlogits are then held against fp64 of the fp32 logits as in the test above.
    Guard words stay.  M = 513 and N = 33 are DS_ERR_ARG before any launch."""
    from tumblr_emotions_amd import _lib
    ops = _ops()
    lib = _lib.load()
    worst = HR.Worst()
    splits = 8

    def fused(ce, sd, bd, yd, N):
        got = [torch.full((M * N + 4,), GUARD, device="cuda"), torch.full((2,), GUARD, device="cuda"),
               torch.full((M * N + 4,), GUARD, device="cuda")]
        _lib.check(lib.ds_slab_epilogue_ce_opts(None if ce is None else C.byref(ce), ops._p(sd), splits, M * N, N, M, N,
                                                ops._p(got[0]), ops._p(bd), ops._p(yd), 1.0, None, ops._p(got[1]), ops._p(got[2]),
                                                ops._stream()), "ds_slab_epilogue_ce_opts")
        torch.cuda.synchronize()
        got = [host(g) for g in got]
        assert (got[0][M * N:] == GUARD).all() and got[1][1] == GUARD and (got[2][M * N:] == GUARD).all(), (M, N)
        return got[0][:M * N].reshape(M, N), got[1][:1], got[2][:M * N].reshape(M, N)

    for N in (1, 15, 32):
        rng = np.random.RandomState(M + N)
        slabs = rng.normal(size=(splits, M, N)).astype(np.float32)
        bias = rng.normal(size=N).astype(np.float32)
        y = rng.randint(0, N, size=M)
        cw = _weight_settings(np.random.RandomState(M * N), N, y)[2][1]
        sd, bd, yd, cwd = dev(slabs), dev(bias), dev(y, torch.int64), dev(cw)
        what = "ds_slab_epilogue_ce_opts M=%d N=%d" % (M, N)
        ref = [torch.full((M, N), NAN, device="cuda"), torch.full((1,), NAN, device="cuda"), torch.full((M, N), NAN, device="cuda")]
        _lib.check(lib.ds_slab_epilogue(ops._p(sd), splits, M * N, N, M, N, ops._p(ref[0]), N, ops._p(bd), None, 0,
                                        ops.DS_EPI_BIAS, ops._stream()), "ds_slab_epilogue")
        ce = ops.ce_desc(0.1, cwd)
        ops.softmax_ce_opts(ce, ref[0], yd, M, N, 1.0, None, ref[1], ref[2])
        logits, loss, dl = fused(ce, sd, bd, yd, N)
        for g, r, name in zip((logits, loss, dl), ref, ("logits", "loss", "dlogits")):
            HR.check_bits(g, host(r), what + " " + name)
        LR.check_ce(loss, dl, logits, y, 0.1, cw, 1.0, what, worst)
        # the default descriptor: ds_slab_epilogue_ce's bits
        old = [torch.full((M, N), NAN, device="cuda"), torch.full((1,), NAN, device="cuda"), torch.full((M, N), NAN, device="cuda")]
        _lib.check(lib.ds_slab_epilogue_ce(ops._p(sd), splits, M * N, N, M, N, ops._p(old[0]), ops._p(bd), ops._p(yd), 1.0, None,
                                           ops._p(old[1]), ops._p(old[2]), ops._stream()), "ds_slab_epilogue_ce")
        for desc in (ops.ce_desc(0.0, None), None):
            for g, r, name in zip(fused(desc, sd, bd, yd, N), old, ("logits", "loss", "dlogits")):
                HR.check_bits(g, host(r), what + " default descriptor " + name)
    for M_, N_ in ((513, 15), (M, 33)):
        z = torch.zeros(M_ * N_, device="cuda")
        ce = ops.ce_desc(0.1, None)
        rc = lib.ds_slab_epilogue_ce_opts(C.byref(ce), ops._p(torch.zeros(splits * M_ * N_, device="cuda")), splits, M_ * N_, N_,
                                          M_, N_, ops._p(z), None, ops._p(torch.zeros(M_, dtype=torch.int64, device="cuda")), 1.0,
                                          None, None, None, ops._stream())
        assert rc == -1 and b"ds_slab_epilogue_ce_opts" in lib.ds_last_error()      # DS_ERR_ARG
    print("ds_slab_epilogue_ce_opts M=%d: %s" % (M, worst))


# ---- the training step -----------------------------------------------------------------------------------------------------

class LossRef(R.DeepSentimentRef):
    """The oracle model with slim's loss options: loss() returns loss_ref.torch_ce in place of the plain mean."""
    label_smoothing, class_weights = 0.0, None

    def loss(self, logits, labels):
        ce = LR.torch_ce(logits, labels, self.label_smoothing, self.class_weights)
        reg = torch.zeros((), dtype=self.dtype)
        if self.mode != "text":
            for name, w in self.p.items():
                if name.startswith("InceptionV1/") and name.endswith("/weights"):
                    reg = reg + S.WEIGHT_DECAY * 0.5 * (w * w).sum()
        return ce + reg, ce


def _loss_ref(params, emb, mode, **keys):
    ref = LossRef(params, emb, mode, torch.float64)
    ref.label_smoothing, ref.class_weights = keys["label_smoothing"], keys["class_weights"]
    return ref


def test_three_text_steps_follow_the_oracle_with_the_new_loss():
    """Smoothing 0.1 and non-uniform weights with one zero (a class the batch holds): logits, loss, every gradient and the
    variables after Adam at the gates of test_model_gpu._check_step (logits and loss 1e-3, gradients 1e-3 relative L2 and
    max-norm, Adam within 2.5 lr and 1e-5 on the resolved entries), each step from the oracle's state."""
    from tumblr_emotions_amd.net import SentimentNet
    rng = np.random.RandomState(21)
    V, D, H, T, B = 40, 12, 16, 9, 8
    params = R.make_params("text", rng, num_classes=15, embed_dim=D, rnn_size=H, dtype=np.float64)
    params["Text/rnn/basic_lstm_cell/bias"] = rng.normal(0, 0.1, size=4 * H)
    emb = S.synthetic_embedding(V, D).astype(np.float64)
    ref = _loss_ref(params, emb, "text", **KEYS)
    net = SentimentNet(mode="text", nb_emotions=15, rnn_size=H, vocab_size=V, embedding_dim=D, post_size=T, **KEYS)
    net.load_state_dict(dict(params, **{"Text/W_embedding": emb}))
    for i in range(3):
        batch = S.synthetic_batch(B, T, V, seed=3 + i, with_images=False)
        batch["labels"][:3] = (2, 2, 5)      # two rows of the dead class: P < B
        assert 0 < int((np.asarray(CW15)[batch["labels"]] != 0).sum()) < B
        if i:
            _sync_from_oracle(net, ref, emb)
        out = _check_step(net, ref, batch, 1e-3, first=(i == 0))
        plain = float(torch.nn.functional.cross_entropy(out["logits"], torch.as_tensor(batch["labels"])))
        assert abs(out["ce"] - plain) > 1e-2      # (the gates above could not pass on the plain loss)


def test_small_joint_step_through_the_fused_launch_and_without_it(monkeypatch):
    """One joint step at B = 4 (test_joint_step_matches_oracle's dims with the model's own rnn_size, and its gates: gradients
    2e-3 at this batch size, as there) with the keys: grouped head -> ds_slab_epilogue_ce_opts, grouping off -> ds_softmax_ce_opts; the two leave the same bits,
    and the grouped one follows the oracle with the new loss."""
    from tumblr_emotions_amd import _lib
    from tumblr_emotions_amd.net import SentimentNet
    rng = np.random.RandomState(24)
    V, D, H, T, B = 60, 20, 512, 12, 4      # (rnn_size 512: below 256 the head's text GEMMs are not split and nothing is grouped)
    params = R.make_params("joint", rng, num_classes=15, im_features_size=256, embed_dim=D, rnn_size=H, fc_size=512,
                           dtype=np.float64)
    emb = S.synthetic_embedding(V, D).astype(np.float64)
    batch = S.synthetic_batch(B, T, V, seed=6)
    batch["labels"][:] = (2, 6, 0, 13)      # one row of the dead class
    ref, fresh = _loss_ref(params, emb, "joint", **KEYS), _loss_ref(params, emb, "joint", **KEYS)      # (fresh: never stepped)
    calls = []
    check = _lib.check
    monkeypatch.setattr(_lib, "check", lambda rc, what: (calls.append(what), check(rc, what))[1])
    outs = {}
    for on in (True, False):
        net = SentimentNet(mode="joint", nb_emotions=15, im_features_size=256, rnn_size=H, fc_size=512, vocab_size=V,
                           embedding_dim=D, post_size=T, dropout_keep_prob=1.0, **KEYS)
        net.head.group = on
        net.image.head_group = on
        net.load_state_dict(dict(params, **{"Text/W_embedding": emb}))
        # a net's first step builds the head's plans and forms the cross entropy in its own launch (SentimentNet._step_body):
        # one step to get past it, then back to the oracle's state (variables, moving statistics, zero slots, step 0)
        dev_batch = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in batch.items()}
        net.train_step(dev_batch, 1e-3)
        assert net.head.grouped() == on and net.head.ce_fused() == on
        _sync_from_oracle(net, ref if on else fresh, emb)
        del calls[:]
        if on:
            _check_step(net, ref, batch, 1e-3, grad_tol=2e-3)
        else:
            keep_activations(net)      # (what _check_step does before its step: the engine re-allocates, the pivots start over)
            net.train_step(dev_batch, 1e-3)
        torch.cuda.synchronize()
        ce_calls = [c for c in calls if "softmax_ce" in c or "epilogue_ce" in c]
        assert ce_calls == (["ds_slab_epilogue_ce_opts"] if on else ["ds_softmax_ce_opts"]), ce_calls
        outs[on] = [host(x) for x in (net.logits, net.loss_buf, net.dlogits, net.store.grad, net.store.theta)]
    for a, b, what in zip(outs[True], outs[False], ("logits", "loss", "dlogits", "grad", "theta")):
        assert _bits(a, b), what


def _split_labels(batch):
    """Rows 0-3 hold one row of the dead class 2, rows 4-7 three: two clones (or ranks) of 4 rows count P = 3 and P = 1."""
    batch["labels"][:] = np.array([2, 1, 4, 6, 2, 2, 9, 2])
    return batch


def test_two_clones_normalise_by_their_own_count():
    """K = 2 text clones whose sub-batches count P = 3 and P = 1: the gradient is that of the fp64 mean of the two per-clone
    losses (slim computes the loss per clone, model_deploy.py:221-223), composed here from the oracle's forward and the new
    loss.  Dividing by the P of the whole batch instead would weigh the second clone's one counted row three times less."""
    from tumblr_emotions_amd.net import SentimentNet
    rng = np.random.RandomState(27)
    V, D, H, T, B = 40, 12, 16, 9, 8
    params = R.make_params("text", rng, num_classes=15, embed_dim=D, rnn_size=H, dtype=np.float64)
    emb = S.synthetic_embedding(V, D).astype(np.float64)
    batch = _split_labels(S.synthetic_batch(B, T, V, seed=5, with_images=False))
    ref = _loss_ref(params, emb, "text", **KEYS)
    halves = [{k: v[lo:lo + 4] for k, v in batch.items()} for lo in (0, 4)]
    ces = [LR.torch_ce(ref.forward(h), h["labels"], **KEYS) for h in halves]
    w = np.asarray(CW15)[batch["labels"]]
    assert [int((w[lo:lo + 4] != 0).sum()) for lo in (0, 4)] == [3, 1]
    total = (ces[0] + ces[1]) / 2
    total.backward()
    net = SentimentNet(mode="text", nb_emotions=15, rnn_size=H, vocab_size=V, embedding_dim=D, post_size=T, **KEYS)
    net.load_state_dict(dict(params, **{"Text/W_embedding": emb}))
    net.train_step({k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in batch.items()}, 1e-3, num_clones=2)
    assert abs(net.total_loss_value() - float(total.detach())) <= 1e-3
    clone_ce = net.clone_loss.cpu().numpy()
    for c in range(2):
        assert abs(clone_ce[c] - float(ces[c].detach())) <= 1e-3, c
    grads = net.grads_state_dict()      # the SUM of the clone gradients: 1 / K is applied inside Adam
    for name in ref.trainable:
        _grad_close(grads[name] / 2, ref.p[name].grad.numpy(), "gradient of " + name)
    # ... and it is not the gradient of the loss normalised over the whole batch
    whole = _loss_ref(params, emb, "text", **KEYS)
    LR.torch_ce(whole.forward(batch), batch["labels"], **KEYS).backward()
    with pytest.raises(AssertionError):
        _grad_close(grads["W_softmax"] / 2, whole.p["W_softmax"].grad.numpy(), "W_softmax against the whole-batch loss")


def _dp_loss_worker(rank, world, port, out):
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    from tumblr_emotions_amd import dp
    dp.init_distributed("gloo", device=0, rank=rank, world_size=world)
    try:
        from tumblr_emotions_amd.net import SentimentNet
        from tumblr_emotions_amd.synthetic import synthetic_batch_numpy, to_device
        net = SentimentNet(mode="text", **dict(TEXT, **KEYS))
        net.initialize(seed=3)
        for i in range(2):
            gb = _split_labels(synthetic_batch_numpy(8, 10, 50, seed=4 + i, with_images=False))
            net.train_step(to_device(gb, "cuda", rank, world), 1e-3)
        torch.cuda.synchronize()
        out.put((rank, [x.cpu().numpy() for x in (net.store.theta, net.store.m, net.store.v)], net.total_loss_value()))
    finally:
        dist.destroy_process_group()


def test_two_ranks_end_where_two_clones_end():
    """Two ranks of 4 rows (P = 3 and P = 1), each normalising by its own count, against one process with two clones of the
    same rows: DESIGN.md 7.12 states this pairing bit for bit for the text model (no BatchNorm, no dropout, a two-term fp32
    sum does not depend on its order), and so it is held here: theta and both Adam slots after two steps."""
    from tumblr_emotions_amd.synthetic import synthetic_batch_numpy, to_device
    ctx = mp.get_context("spawn")
    out = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_dp_loss_worker, args=(r, 2, port, out)) for r in range(2)]
    for p in procs:
        p.start()
    net = _net(**KEYS)
    for i in range(2):
        gb = _split_labels(synthetic_batch_numpy(8, 10, 50, seed=4 + i, with_images=False))
        net.train_step(to_device(gb), 1e-3, num_clones=2)
    torch.cuda.synchronize()
    mine = [x.cpu().numpy() for x in (net.store.theta, net.store.m, net.store.v)]
    clone_ce = net.clone_loss.cpu().numpy()
    got = {r: (state, loss) for r, state, loss in _collect(out, procs, 2)}
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    for a, b, c, what in zip(got[0][0], got[1][0], mine, ("theta", "m", "v")):
        assert np.array_equal(a, b) and np.array_equal(a, c), what
    assert not np.array_equal(mine[1], np.zeros_like(mine[1]))
    # each rank's loss is its clone's, normalised by its own P
    for r in range(2):
        assert got[r][1] == float(clone_ce[r]), r


@pytest.mark.parametrize("mode", ["text", "joint"])
def test_three_replays_of_a_captured_step_equal_three_eager_steps(mode):
    """... bit for bit, in the text model (ds_softmax_ce_opts) and the joint model (ds_slab_epilogue_ce_opts).  The host
    descriptor is overwritten after the capture: a replay reads nothing of it (the smoothing is a kernel argument of the
    captured launch, the weights are read from their device buffer)."""
    batch = _batch(0, mode)
    dims = dict(rnn_size=512) if mode == "joint" else {}      # (the model's own: the grouped head, the fused launch)
    outs = []
    for graphed in (False, True):
        net = _net(mode, **dict(KEYS, **dims))
        if graphed:
            assert net.capture_step(batch)
            net.ce_desc.label_smoothing = 0.5
            net.ce_desc.class_weights = None
        for i in range(3):
            net.train_step(batch, 1e-3)
        assert (net._graph is not None) == graphed and net.step == 3
        assert mode != "joint" or (net.head.grouped() and net.head.ce_fused())
        torch.cuda.synchronize()
        outs.append([host(x) for x in (net.store.theta, net.store.m, net.store.v, net.loss_buf, net.dlogits, net.logits)])
    for a, b, what in zip(outs[0], outs[1], ("theta", "m", "v", "loss", "dlogits", "logits")):
        assert _bits(a, b), what
    LR.check_ce(outs[0][3], outs[0][4], outs[0][5], host(batch["labels"]), 0.1, np.asarray(CW15, np.float32), 1.0,
                "the last %s step" % mode)


@pytest.mark.parametrize("mode", ["text", "image", "joint"])
def test_keys_absent_or_zero_smoothing_alone_is_the_step_without_them(mode, monkeypatch):
    """Keys absent, label_smoothing = None and label_smoothing = 0.0 alone: no descriptor, no device buffer, the launch names
    of the step without the arguments (ds_softmax_ce / ds_slab_epilogue_ce and no _opts entry), and theta, both slots and the
    loss after three steps bit-identical to a net built without the arguments.  With the keys the one cross-entropy launch
    is the _opts form, and its loss and dlogits are the reference's of the step's own logits -- in all three modes."""
    from tumblr_emotions_amd import _lib
    calls = []
    check = _lib.check
    monkeypatch.setattr(_lib, "check", lambda rc, what: (calls.append(what), check(rc, what))[1])
    rows = 8 if mode == "text" else 4
    dims = dict(rnn_size=512) if mode == "joint" else {}      # (the model's own: the grouped head, the fused launch)
    runs = {}
    for name, kw in (("without", {}), ("none", dict(label_smoothing=None, class_weights=None)), ("zero", dict(label_smoothing=0.0)),
                     ("keys", KEYS)):
        net = _net(mode, **dict(kw, **dims))
        assert (net.ce_desc is None and net.class_weights_dev is None) == (name != "keys")
        del calls[:]
        for i in range(3):
            net.train_step(_batch(i, mode, rows=rows), 1e-3)
        loss = net.total_loss_value()
        runs[name] = (list(calls), [host(x) for x in (net.store.theta, net.store.m, net.store.v)], loss)
        ce_calls = [c for c in calls if "softmax_ce" in c or "epilogue_ce" in c]
        # (a joint net's first step builds the head's plans and forms the cross entropy in its own launch, the next ones in the
        # W_softmax combine: SentimentNet._step_body)
        old = ["ds_softmax_ce", "ds_slab_epilogue_ce", "ds_slab_epilogue_ce"] if mode == "joint" else ["ds_softmax_ce"] * 3
        assert ce_calls == [c + "_opts" if name == "keys" else c for c in old], (name, ce_calls)
        if name == "keys":
            LR.check_ce(host(net.loss_buf), host(net.dlogits), host(net.logits), host(_batch(2, mode, rows=rows)["labels"]), 0.1,
                        np.asarray(CW15, np.float32), 1.0, "the third %s step" % mode)
    for name in ("none", "zero"):
        assert runs[name][0] == runs["without"][0], name
        assert all(_bits(a, b) for a, b in zip(runs[name][1], runs["without"][1])) and runs[name][2] == runs["without"][2], name
    assert [c for c in runs["keys"][0] if not c.endswith("_opts")] == [c for c in runs["without"][0] if c not in ("ds_softmax_ce", "ds_slab_epilogue_ce")]
    assert not _bits(runs["keys"][1][0], runs["without"][1][0]) and runs["keys"][2] != runs["without"][2]


@pytest.mark.parametrize("dtype", ["bf16", "fp8"])
def test_sixteen_bit_and_fp8_configurations_hand_over_fp32_logits_and_are_not_refused(dtype):
    """The 16-bit and fp8 labels change the conv arithmetic and the activation storage; the logits and dlogits stay fp32, so the
    keys are not refused there: one image step, the loss and dlogits held against the reference of the step's own logits."""
    net = _net("image", dtype=dtype, **KEYS)
    batch = _batch(0, "image", rows=4)
    net.train_step(batch, 1e-3)
    torch.cuda.synchronize()
    assert net.logits.dtype == torch.float32 and net.dlogits.dtype == torch.float32
    LR.check_ce(host(net.loss_buf), host(net.dlogits), host(net.logits), host(batch["labels"]), 0.1, np.asarray(CW15, np.float32),
                1.0, "an image step in %s" % dtype)
    assert np.isfinite(host(net.store.theta)).all()


# ---- the front end -------------------------------------------------------------------------------------------------------

def _lines(path):
    with open(path) as f:
        return [json.loads(l) for l in f if l.strip()]


def test_train_and_evaluate_text_model_with_both_keys(tmp_path):
    """train_text_model with both keys for three steps and validation every two: the checkpoint carries "loss"; the loss the
    run logs is the weighted, smoothed one (recomputed in fp64 from the logits of a model restored from the two-step run's
    checkpoint -- training runs are bit-reproducible -- on the third batch); validation.jsonl keeps the plain mean cross
    entropy (recomputed from the final checkpoint's logits on the validation batches); evaluate_text_model ignores the keys;
    a run without them writes no "loss"."""
    from tumblr_emotions_amd.text_model.text_embedding import TextModel, _CONFIG, evaluate_text_model, train_text_model
    from tumblr_emotions_amd.training import load_checkpoint
    cfg = dict(SMALL_TEXT, validate_every=2, validate_batches=2, **KEYS)
    dirs = {k: str(tmp_path / k) for k in ("three", "two", "plain")}
    logged = train_text_model(dirs["three"], 3, config=cfg, quiet=True)
    train_text_model(dirs["two"], 2, config=cfg, quiet=True)
    ck = torch.load(os.path.join(dirs["three"], "model.ckpt-3.pt"), map_location="cpu", weights_only=True)
    assert ck["loss"] == {"label_smoothing": 0.1, "class_weights": [float(w) for w in CW15]}
    # the logged loss: the third step's, from the state the second step left
    model = TextModel(dict(_CONFIG, **SMALL_TEXT))
    assert model.net.ce_desc is None
    load_checkpoint(model, os.path.join(dirs["two"], "model.ckpt-2.pt"))
    batch = model.next_batch(2)
    labels = host(batch["labels"])
    logits = host(model.net.predict(batch, is_training=False)).astype(np.float64)
    want, _ = LR.softmax_ce(logits, labels, 0.1, CW15)
    plain, _ = HR.softmax_ce(logits.copy(), labels)
    assert abs(logged - want) <= 1e-5 * want and abs(want - plain) > 1e-2 * plain, (logged, want, plain)
    # validation: the plain mean cross entropy of the held-out batches, at steps 2 and 3
    lines = _lines(os.path.join(dirs["three"], "validation.jsonl"))
    assert [l["global_step"] for l in lines] == [2, 3]
    for line, d, step in ((lines[0], "two", 2), (lines[1], "three", 3)):
        load_checkpoint(model, os.path.join(dirs[d], "model.ckpt-%d.pt" % step))
        rows = []
        for vb in model.validation_batches(2):
            z = host(model.net.predict(vb, is_training=False)).astype(np.float64)
            rows.append(np.log(np.exp(z - z.max(1, keepdims=True)).sum(1)) + z.max(1) - z[np.arange(len(z)), host(vb["labels"])])
        plain_val = float(np.concatenate(rows).mean())
        weighted_val = np.mean([LR.softmax_ce(host(model.net.predict(vb, is_training=False)).astype(np.float64),
                                              host(vb["labels"]), 0.1, CW15)[0] for vb in model.validation_batches(2)])
        assert line["n"] == 16 and abs(line["loss"] - plain_val) <= 1e-5 * plain_val, (line, plain_val)
        assert abs(weighted_val - plain_val) > 1e-3 * plain_val
    # evaluation ignores the keys; a run without them has the checkpoint keys it had
    acc = evaluate_text_model(dirs["three"], str(tmp_path / "log"), "validation", 2, config=cfg, quiet=True)
    assert acc == evaluate_text_model(dirs["three"], str(tmp_path / "log2"), "validation", 2, config=SMALL_TEXT, quiet=True)
    train_text_model(dirs["plain"], 1, config=dict(SMALL_TEXT, label_smoothing=0.0), quiet=True)
    assert "loss" not in torch.load(os.path.join(dirs["plain"], "model.ckpt-1.pt"), map_location="cpu", weights_only=True)
    # a bad key is refused by the trainer before a model exists
    with pytest.raises(ValueError, match="class_weights"):
        train_text_model(dirs["plain"], 1, config=dict(SMALL_TEXT, class_weights=[0.0] * 15), quiet=True)
    with pytest.raises(ValueError, match="exactly nb_emotions"):
        train_text_model(dirs["plain"], 1, config=dict(SMALL_TEXT, class_weights=[1.0] * 3), quiet=True)
