"""Several clones per GPU (SentimentNet.train_step(num_clones=K)): the accumulation kernel against NumPy, the
clone step against the oracle's definition of slim's in-graph clones (DeepSentimentRef.train_step_dp), its bit-for-bit
relations to the plain step and to data parallelism, the front-end key and the refused combinations."""
import json
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from oracle import tf_semantics as S
from oracle import torch_ref as R

from test_dp_gpu import DP_LR, DP_PER_RANK, JOINT, TEXT, _collect, _dp_parity_inputs, _free_port
from test_model_gpu import _dev_batch, _grad_close, _sync_from_oracle

pytestmark = pytest.mark.gpu

V, D, H, T = 40, 12, 16, 9            # the dims of test_text_only_step_matches_oracle
SMALL = dict(nb_emotions=15, rnn_size=H, vocab_size=V, embedding_dim=D, post_size=T)


# ---- a. the kernel ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [4, 1028, (1 << 20) + 4])
def test_grad_accumulate_sums_three_clones_in_order(n):
    """n = 4: one thread's worth; 1028: a ragged tail against the block; 2^20 + 4: more than one trip of the grid-stride
    loop.  Three 'clones' through modes 0, 1, 2: NumPy's (g0 + g1) + g2 in float32, bit for bit; mode 2 writes g and leaves
    acc; nothing past n is touched."""
    from tumblr_emotions_amd import ops
    rng = np.random.RandomState(n % 1000)
    pad = 8
    gs = [(rng.standard_normal(n) * 10.0 ** rng.uniform(-6, 6, size=n)).astype(np.float32) for _ in range(3)]
    acc = torch.full((n + pad,), -7.0, device="cuda")
    g = torch.full((n + pad,), 3.0, device="cuda")
    want = gs[0].copy()
    for c in range(3):
        g[:n].copy_(torch.from_numpy(gs[c]))
        acc_before = acc.clone()
        ops.grad_accumulate(acc, g, n, c)
        torch.cuda.synchronize()
        if c:
            want = want + gs[c]
        assert want.dtype == np.float32
        if c < 2:
            assert np.array_equal(acc[:n].cpu().numpy(), want), c
            assert np.array_equal(g[:n].cpu().numpy(), gs[c]), c                 # modes 0 and 1 only read g
        else:
            assert torch.equal(acc, acc_before)                                  # mode 2 only reads acc
            assert np.array_equal(g[:n].cpu().numpy(), want)
        assert bool((acc[n:] == -7.0).all()) and bool((g[n:] == 3.0).all()), c
    assert np.array_equal(want, (gs[0] + gs[1]) + gs[2])


# ---- the text problem of b, f ------------------------------------------------------------------------------------------
def _text_problem(B, seed):
    rng = np.random.RandomState(seed)
    params = R.make_params("text", rng, num_classes=15, embed_dim=D, rnn_size=H, dtype=np.float64)
    params["Text/rnn/basic_lstm_cell/bias"] = rng.normal(0, 0.1, size=4 * H)
    emb = S.synthetic_embedding(V, D).astype(np.float64)
    batch = S.synthetic_batch(B, T, V, seed=seed + 1, with_images=False)
    return params, emb, batch


def _check_text_clones(got, o, ref, n_clones_total, my_clones, lr, first):
    """The gates of test_model_gpu._check_step for a step of clones: `got` = dict(logits [rows of my clones], loss, grads
    (the summed buffer), after), o = train_step_dp's result over ALL clones, my_clones = their indices in o."""
    b = got["logits"].shape[0] // len(my_clones)
    for i, c in enumerate(my_clones):
        err = np.abs(got["logits"][i * b:(i + 1) * b] - o["logits"][c].numpy()).max()
        assert err <= 1e-3, "clone %d: logits differ by %.3e" % (c, err)
    want_loss = (o["loss"] - np.mean(o["ce"])) + np.mean([o["ce"][c] for c in my_clones])      # L2 term + MY clones' mean CE
    assert abs(got["loss"] - want_loss) <= 1e-3, (got["loss"], want_loss)
    assert set(got["grads"]) >= set(o["grads"])
    for name, g_ref in o["grads"].items():
        _grad_close(got["grads"][name] / float(n_clones_total), g_ref.numpy(), "gradient of " + name, 1e-3)
    for name in ref.trainable:
        w_ref = ref.p[name].detach().numpy()
        w = got["after"][name].reshape(w_ref.shape)
        assert np.abs(w - w_ref).max() <= 2.5 * lr + 1e-6, name
        if first:
            g_ref = o["grads"][name].numpy()
            big = np.abs(g_ref) > 1e-2 * max(np.abs(g_ref).max(), 1e-12)
            if big.any():
                d_big = np.abs(w - w_ref)[big]
                assert (d_big <= 1e-5).mean() >= 0.99, "%s: %.4f of the well-resolved entries within 1e-5 (worst %.3e)" % (
                    name, (d_big <= 1e-5).mean(), d_big.max())


def _result(net):
    torch.cuda.synchronize()
    return dict(logits=net.logits.detach().cpu().numpy(), loss=net.total_loss_value(), grads=net.grads_state_dict(),
                after=net.state_dict())


# ---- b. text, K = 3 ------------------------------------------------------------------------------------------------------
def test_text_three_clones_match_the_clone_oracle():
    """K = 3 is the smallest count that runs all three kernel modes.  Two steps, the second from the oracle's optimiser
    state (non-zero Adam slots), the shortest and the full-length post in different clones."""
    from tumblr_emotions_amd.net import SentimentNet
    K, B, lr = 3, 12, 1e-3
    params, emb, batch = _text_problem(B, 21)
    batch["seq_lens"][0], batch["seq_lens"][5] = 1, T          # clone 0 / clone 1
    batch["texts"][0, 1:] = V
    batch["texts"][5] = np.arange(T) % V
    ref = R.DeepSentimentRef(params, emb, "text", torch.float64)
    net = SentimentNet(mode="text", **SMALL)
    net.load_state_dict(dict(params, **{"Text/W_embedding": emb}))
    subs = [{k: v[c * 4:(c + 1) * 4] for k, v in batch.items()} for c in range(K)]
    dev = _dev_batch(batch)
    for i in range(2):
        if i:
            _sync_from_oracle(net, ref, emb)
        calls = []
        net.train_step(dev, lr, num_clones=K, after_clone=calls.append)
        assert calls == [0, 1, 2] and net.step == i + 1 == ref.step + 1
        assert tuple(net.logits.shape) == (B, 15)
        o = ref.train_step_dp(subs, lr)
        _check_text_clones(_result(net), o, ref, K, [0, 1, 2], lr, first=(i == 0))


# ---- c. joint, K = 2 x 8 rows -----------------------------------------------------------------------------------------------
def test_joint_two_clones_match_the_clone_oracle_and_clone_0_owns_the_moving_statistics():
    """The inputs and gates of test_dp_gpu.test_two_rank_joint_step_matches_the_clone_oracle, with the two clones on one net.
    Then the exact statement: clone 0 ran the launches of a plain step on rows [0, 8) from the same state and the same
    pivots, so the moving statistics are that step's, bit for bit -- and not those of rows [8, 16)."""
    from hip_decisions import hip_decisions, keep_activations
    from tumblr_emotions_amd.net import SentimentNet
    params, emb, batch = _dp_parity_inputs()
    n = DP_PER_RANK
    assert batch["labels"].shape[0] == 2 * n == 16
    dev = _dev_batch(batch)

    def fresh():
        net = SentimentNet(mode="joint", dropout_keep_prob=1.0, **JOINT)
        net.load_state_dict(dict(params, **{"Text/W_embedding": emb}))
        keep_activations(net)
        return net

    net = fresh()
    seen = []

    def after_clone(c):
        torch.cuda.synchronize()
        seen.append((c, hip_decisions(net), net.logits.detach().cpu().numpy()))

    net.train_step(dev, DP_LR, num_clones=2, after_clone=after_clone)
    torch.cuda.synchronize()
    assert [s[0] for s in seen] == [0, 1] and net.step == 1
    got = _result(net)
    l2 = [e.name for e in net.store.entries.values() if e.trainable and e.l2]
    subs = [{k: v[c * n:(c + 1) * n] for k, v in batch.items()} for c in range(2)]
    ref = R.DeepSentimentRef(params, emb, "joint", torch.float64)
    with torch.no_grad():
        plain = [ref.forward(s).detach().clone() for s in subs]
    o = ref.train_step_dp(subs, DP_LR, injects=[seen[0][1], seen[1][1]])
    for c in range(2):
        assert float((o["logits"][c] - plain[c]).abs().max()) <= 1e-4
        assert np.abs(seen[c][2] - o["logits"][c].numpy()).max() <= 1e-3, c
        assert np.array_equal(got["logits"][c * n:(c + 1) * n], seen[c][2]), c       # net.logits: all rows, in order
    assert abs(got["loss"] - o["loss"]) <= 1e-3, (got["loss"], o["loss"])
    assert len(o["grads"]) == 71
    worst = (0.0, "")
    for name, g_ref in o["grads"].items():
        g_ref = g_ref.numpy()
        g = got["grads"][name].reshape(g_ref.shape) / 2.0
        if name in l2:
            g = g + 0.00004 * params[name]
        d = g - g_ref
        rel = np.linalg.norm(d) / max(np.linalg.norm(g_ref), 1e-30)
        emax = np.abs(d).max() / max(np.abs(g_ref).max(), 1e-30)
        worst = max(worst, (rel, name))
        assert rel <= 1e-3 and emax <= 1e-3, "gradient of %s: relative L2 %.3e, max-norm %.3e" % (name, rel, emax)
    print("two clones, worst gradient relative L2 against the clone oracle: %.3e (%s)" % worst)
    for name in ref.trainable:
        w_ref = ref.p[name].detach().numpy()
        g_ref = o["grads"][name].numpy()
        big = np.abs(g_ref) > 1e-2 * max(np.abs(g_ref).max(), 1e-12)
        assert (np.abs(got["after"][name].reshape(w_ref.shape) - w_ref)[big] <= 1e-5).mean() >= 0.99, name
    moving = [k for k in got["after"] if k.endswith("moving_mean") or k.endswith("moving_variance")]
    assert len(moving) == 2 * 57
    for name in moving:
        np.testing.assert_allclose(got["after"][name], ref.p[name].numpy(), atol=1e-5, err_msg=name)
    # the exact check
    first, second = fresh(), fresh()
    first.train_step({k: v[:n] for k, v in dev.items()}, DP_LR)
    second.train_step({k: v[n:].clone() for k, v in dev.items()}, DP_LR)
    a, b = first.state_dict(), second.state_dict()
    for name in moving:
        assert np.array_equal(got["after"][name], a[name]), name
    assert any(not np.array_equal(got["after"][name], b[name]) for name in moving)


# ---- d. K = 1 is today's step ------------------------------------------------------------------------------------------------
def test_one_clone_is_the_plain_step_bit_for_bit():
    from tumblr_emotions_amd.net import SentimentNet
    from tumblr_emotions_amd.synthetic import synthetic_batch_numpy, to_device
    batch = to_device(synthetic_batch_numpy(8, 10, 50, seed=4, with_images=True))
    nets = []
    for kw in ({"num_clones": 1}, {}):
        net = SentimentNet(mode="joint", dropout_keep_prob=0.8, **TEXT)
        net.initialize(seed=3)
        for i in range(3):
            net.train_step(batch, 1e-3, **kw)
        torch.cuda.synchronize()
        nets.append(net)
    one, plain = nets
    sa, sb = one.state_dict(), plain.state_dict()
    assert sorted(sa) == sorted(sb)
    for k in sa:
        assert np.array_equal(sa[k], sb[k]), k
    assert torch.equal(one.store.m, plain.store.m) and torch.equal(one.store.v, plain.store.v)
    assert len(one.image.layers) == len(plain.image.layers) > 0      # (the fused 1x1 convs of a block are one layer)
    for la, lb in zip(one.image.layers, plain.image.layers):
        assert torch.equal(la.mean, lb.mean)
    assert torch.equal(one.logits, plain.logits) and one.total_loss_value() == plain.total_loss_value()
    assert getattr(one, "grad_acc", None) is None and getattr(one, "clone_loss", None) is None      # nothing was allocated


# ---- e. text, bit for bit against data parallelism ----------------------------------------------------------------------------
def _state(net):
    torch.cuda.synchronize()
    return dict(net.state_dict(), adam_m=net.store.m.cpu().numpy(), adam_v=net.store.v.cpu().numpy())


def _dp_text_worker(rank, world, port, out):
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    from tumblr_emotions_amd import dp
    dp.init_distributed("gloo", device=0, rank=rank, world_size=world)
    try:
        from tumblr_emotions_amd.net import SentimentNet
        from tumblr_emotions_amd.synthetic import synthetic_batch_numpy, to_device
        net = SentimentNet(mode="text", **TEXT)
        net.initialize(seed=3)
        states = []
        for i in range(3):
            local = to_device(synthetic_batch_numpy(8, 10, 50, seed=4 + i, with_images=False), "cuda", rank, world)
            net.train_step(local, 1e-3)
            states.append(_state(net))
        if rank == 0:
            out.put(states)
    finally:
        dist.destroy_process_group()


def test_text_two_clones_equal_rank_0_of_a_two_rank_run_bit_for_bit():
    """No BatchNorm, no dropout, and a two-term fp32 sum does not depend on its order: one process with K = 2 on 8 rows takes
    the steps of rank 0 of a two-rank run on the same rows."""
    from tumblr_emotions_amd.net import SentimentNet
    from tumblr_emotions_amd.synthetic import synthetic_batch_numpy, to_device
    ctx = mp.get_context("spawn")
    out = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_dp_text_worker, args=(r, 2, port, out)) for r in range(2)]
    for p in procs:
        p.start()
    net = SentimentNet(mode="text", **TEXT)
    net.initialize(seed=3)
    mine = []
    for i in range(3):
        net.train_step(to_device(synthetic_batch_numpy(8, 10, 50, seed=4 + i, with_images=False)), 1e-3, num_clones=2)
        mine.append(_state(net))
    (theirs,) = _collect(out, procs, 1)
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    for i in range(3):
        assert sorted(mine[i]) == sorted(theirs[i])
        for k in mine[i]:
            assert np.array_equal(mine[i][k], theirs[i][k]), (i, k)


# ---- f. 2 ranks x K = 2 -----------------------------------------------------------------------------------------------------
F_SEED, F_LR = 33, 1e-3


def _dp_clones_worker(rank, world, port, out):
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    from tumblr_emotions_amd import dp
    dp.init_distributed("gloo", device=0, rank=rank, world_size=world)
    try:
        from tumblr_emotions_amd.net import SentimentNet
        params, emb, batch = _text_problem(16, F_SEED)
        net = SentimentNet(mode="text", **SMALL)
        assert net.world == world and net.reducer.active
        net.load_state_dict(dict(params, **{"Text/W_embedding": emb}))
        local = _dev_batch({k: v[rank * 8:(rank + 1) * 8] for k, v in batch.items()})
        net.train_step(local, F_LR, num_clones=2)
        assert net.reducer._pending is None and not net.reducer._ready      # deferred: no early bucket-1 launch
        out.put((rank, _result(net)))
    finally:
        dist.destroy_process_group()


def test_two_ranks_of_two_clones_match_the_oracle_over_four_sub_batches():
    ctx = mp.get_context("spawn")
    out = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_dp_clones_worker, args=(r, 2, port, out)) for r in range(2)]
    for p in procs:
        p.start()
    got = dict(_collect(out, procs, 2))
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    for name in got[0]["after"]:
        assert np.array_equal(got[0]["after"][name], got[1]["after"][name]), name
    for name in got[0]["grads"]:
        assert np.array_equal(got[0]["grads"][name], got[1]["grads"][name]), name      # one all-reduced buffer
    params, emb, batch = _text_problem(16, F_SEED)
    subs = [{k: v[i * 4:(i + 1) * 4] for k, v in batch.items()} for i in range(4)]      # (r, c) = (0,0), (0,1), (1,0), (1,1)
    ref = R.DeepSentimentRef(params, emb, "text", torch.float64)
    o = ref.train_step_dp(subs, F_LR)
    _check_text_clones(got[0], o, ref, 4, [0, 1], F_LR, first=True)
    _check_text_clones(got[1], o, ref, 4, [2, 3], F_LR, first=True)


# ---- g. the front end -------------------------------------------------------------------------------------------------------
def test_train_text_model_with_two_clones(tmp_path):
    from tumblr_emotions_amd.net import SentimentNet
    from tumblr_emotions_amd.synthetic import synthetic_batch_numpy, to_device
    from tumblr_emotions_amd.text_model.text_embedding import train_text_model
    lr = 1e-3
    cfg = dict(synthetic=True, batch_size=4, num_clones=2, num_samples=24, decay_factor=0.5, validate_every=1, initial_lr=lr,
               rnn_size=32, vocab_size=60, embedding_dim=20, post_size=12)
    d = str(tmp_path / "clones")
    train_text_model(d, 4, config=cfg, quiet=True)
    with open(os.path.join(d, "validation.jsonl")) as f:
        lines = [json.loads(l) for l in f if l.strip()]
    assert [l["global_step"] for l in lines] == [1, 2, 3, 4]
    assert [l["learning_rate"] for l in lines] == [lr, lr, lr, lr / 2]      # 24 / (4 * 2): an epoch is three steps
    assert all(l["n"] == 10 * 4 for l in lines)                              # validation batches stay batch_size rows
    ck = torch.load(os.path.join(d, "model.ckpt-4.pt"), map_location="cpu", weights_only=True)
    net = SentimentNet(mode="text", nb_emotions=15, rnn_size=32, vocab_size=60, embedding_dim=20, post_size=12)
    net.initialize(seed=1)
    for step, rate in enumerate([lr, lr, lr, lr / 2]):
        net.train_step(to_device(synthetic_batch_numpy(8, 12, 60, 15, seed=step, with_images=False)), rate, num_clones=2)
    torch.cuda.synchronize()
    mine = net.state_dict()
    assert sorted(mine) == sorted(ck["variables"])
    for k in mine:
        assert np.array_equal(mine[k], ck["variables"][k].numpy()), k


# ---- h. refusals ------------------------------------------------------------------------------------------------------------
def test_refused_combinations_leave_the_step_counter_alone():
    from tumblr_emotions_amd.net import SentimentNet
    from tumblr_emotions_amd.synthetic import synthetic_batch_numpy, to_device
    batch = to_device(synthetic_batch_numpy(8, 10, 50, seed=1, with_images=False))
    net = SentimentNet(mode="text", **TEXT)
    net.initialize(seed=3)
    with pytest.raises(ValueError, match="does not divide"):
        net.train_step(batch, 1e-3, num_clones=3)
    with pytest.raises(ValueError, match="explicit seed"):
        net.train_step(batch, 1e-3, seed=11, num_clones=2)
    for bad in (0, -2, 2.0, True):
        with pytest.raises(ValueError, match="positive int"):
            net.train_step(batch, 1e-3, num_clones=bad)
    assert net.step == 0
    assert net.capture_step(batch)
    with pytest.raises(NotImplementedError, match="captured step"):
        net.train_step(batch, 1e-3, num_clones=2)
    with pytest.raises(NotImplementedError, match="not captured"):
        net.capture_step(batch, num_clones=2)
    assert net.step == 0 and net._graph is not None
    sync = SentimentNet(mode="joint", sync_bn=True, **TEXT)
    with pytest.raises(ValueError, match="sync_bn"):
        sync.train_step(batch, 1e-3, num_clones=2)
    half = SentimentNet(mode="joint", dtype="bf16", **TEXT)
    with pytest.raises(NotImplementedError, match="bf16"):
        half.train_step(batch, 1e-3, num_clones=2)
    assert sync.step == 0 and half.step == 0
