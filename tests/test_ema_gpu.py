"""Moving averages of the trained variables on the GPU: ds_adam_tf_ema and ds_adam_tf_clipped_ema against
the existing Adam kernels (bit for bit) and the fp32 / fp64 restatement of TF's update (tests/ema_ref.py), then the training
step, averaged_weights() and the text front end.  Every step test compares bits: the Adam side with a net that has no
moving averages, the shadows with the fp32 recurrence run on the net's own theta."""
import json
import math
import os
from fractions import Fraction

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import ema_ref as E
from test_dp_gpu import TEXT, _collect, _free_port
from test_frontends_gpu import SMALL_TEXT
from test_grad_clip_gpu import Case

pytestmark = pytest.mark.gpu

B1, B2, EPS = 0.9, 0.999, 1e-8
WD, SCALE = 0.25, 0.5
GRID_PASS = 2048 * 256            # elements of one grid-stride pass of ds_adam_tf: stream_grid caps the grid at 8 blocks per CU
SIZES = (4, 1020, 1028, GRID_PASS + 260)
RATE_1 = E.rate32(0.9999, 1)      # 9/11 in fp32 arithmetic
RATES = (RATE_1, E.rate32(0.9999, 10 ** 6), np.float32(0.01))


def _bits(a, b):
    a, b = (x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x) for x in (a, b))
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _magnitudes(rng, n, positive=False):
    x = 10.0 ** rng.uniform(-6, 1, size=n)
    return (x if positive else x * rng.choice([-1.0, 1.0], size=n)).astype(np.float32)


class Flat:
    """theta, g, m, v >= 0 and shadow of n elements with magnitudes 1e-6 .. 10; n_wd ends in the middle of a 256-thread
    block (of the last block that has a middle)."""

    def __init__(self, n, seed):
        rng = np.random.RandomState(seed)
        self.n = n
        self.n_wd = 2 if n < 512 else (n // 256 - 1) * 256 + 100
        assert 0 < self.n_wd < n and (n < 512 or self.n_wd % 256 == 100)
        self.theta, self.g, self.m = (_magnitudes(rng, n) for _ in range(3))
        self.v = _magnitudes(rng, n, positive=True)
        self.shadow = _magnitudes(rng, n)

    def dev(self):
        return [torch.from_numpy(x.copy()).cuda() for x in (self.theta, self.g, self.m, self.v, self.shadow)]


# =========================================================================================================================
# the kernels
# =========================================================================================================================
@pytest.mark.parametrize("n", SIZES)
def test_adam_tf_ema_has_adams_bits_and_tfs_shadow(n):
    from tumblr_emotions_amd import ops
    c = Flat(n, seed=n % 1000)
    lr_t = 3e-3
    theta0, g0, m0, v0, _ = c.dev()
    ops.adam_tf(theta0, g0, m0, v0, n, c.n_wd, WD, SCALE, lr_t, B1, B2, EPS)
    torch.cuda.synchronize()
    assert not _bits(theta0, c.theta)
    worst = 0.0
    for rate in RATES:
        theta, g, m, v, shadow = c.dev()
        ops.adam_tf_ema(theta, g, m, v, shadow, n, c.n_wd, WD, SCALE, lr_t, float(rate), B1, B2, EPS)
        torch.cuda.synchronize()
        for a, b, what in ((theta, theta0, "theta"), (m, m0, "m"), (v, v0, "v"), (g, c.g, "g")):
            assert _bits(a, b), (what, float(rate))
        got, new = shadow.cpu().numpy(), theta.cpu().numpy()
        assert _bits(got, E.update32(c.shadow, new, rate)), float(rate)
        assert not _bits(got, c.shadow)
        err, bound = np.abs(got.astype(np.float64) - E.update64(c.shadow, new, rate)), E.bound64(c.shadow, new, rate)
        worst = max(worst, float((err / bound).max()))
        assert (err <= bound).all(), (float(rate), float((err / bound).max()))
    print("n = %d: largest |error| / bound against fp64 = %.5f" % (n, worst))
    # the rate in device memory overrides the argument; lr_t's device scalar still works beside it
    rate = RATES[0]
    theta, g, m, v, shadow = c.dev()
    ops.adam_tf_ema(theta, g, m, v, shadow, n, c.n_wd, WD, SCALE, 1e3, 0.0, B1, B2, EPS,
                    lr_t_dev=torch.full((1,), lr_t, device="cuda"), ema_rate_dev=torch.full((1,), float(rate), device="cuda"))
    torch.cuda.synchronize()
    assert _bits(theta, theta0) and _bits(m, m0) and _bits(v, v0)
    assert _bits(shadow, E.update32(c.shadow, theta.cpu().numpy(), rate))
    # rate 0: the shadows keep their bits, Adam still steps
    theta, g, m, v, shadow = c.dev()
    ops.adam_tf_ema(theta, g, m, v, shadow, n, c.n_wd, WD, SCALE, lr_t, 0.0, B1, B2, EPS)
    torch.cuda.synchronize()
    assert _bits(shadow, c.shadow) and _bits(theta, theta0)
    # rate 1: the shadow IS the new variable wherever s - (s - w) is exact; everywhere it follows the formula
    theta, g, m, v, shadow = c.dev()
    ops.adam_tf_ema(theta, g, m, v, shadow, n, c.n_wd, WD, SCALE, lr_t, 1.0, B1, B2, EPS)
    torch.cuda.synchronize()
    assert _bits(shadow, E.update32(c.shadow, theta.cpu().numpy(), 1.0))


@pytest.fixture(scope="module")
def case():
    c = Case()
    c.shadow = _magnitudes(np.random.RandomState(5), c.n)
    return c


def _clipped_ema(case, factors, flags, lr_t, rate, rate_dev=None):
    from tumblr_emotions_amd import ops
    theta, m, v = case.state()
    shadow = torch.from_numpy(case.shadow.copy()).cuda()
    ops.adam_tf_clipped_ema(theta, torch.from_numpy(case.g).cuda(), m, v, shadow, case.n, case.n_wd, WD, SCALE, lr_t, rate, B1, B2,
                            EPS, case.seg, case.chunks, factors, flags, ema_rate_dev=rate_dev)
    torch.cuda.synchronize()
    return [x.cpu().numpy() for x in (theta, m, v, shadow)]


def test_clipped_ema_with_unit_factors_has_the_bits_of_adam_tf_ema(case):
    from tumblr_emotions_amd import ops
    lr_t, rate = 3e-3, float(RATE_1)
    flags = torch.zeros(4, dtype=torch.int32, device="cuda")
    got = _clipped_ema(case, torch.ones(case.nseg + 1, device="cuda"), flags, lr_t, rate)
    theta, m, v = case.state()
    shadow = torch.from_numpy(case.shadow.copy()).cuda()
    ops.adam_tf_ema(theta, torch.from_numpy(case.g).cuda(), m, v, shadow, case.n, case.n_wd, WD, SCALE, lr_t, rate, B1, B2, EPS)
    torch.cuda.synchronize()
    for x, y, what in zip(got, (theta, m, v, shadow), ("theta", "m", "v", "shadow")):
        assert _bits(x, y), what
    assert flags.cpu().tolist() == [0, 0, 0, 0] and not _bits(got[3], case.shadow)
    # ... and from device memory
    again = _clipped_ema(case, torch.ones(case.nseg + 1, device="cuda"), flags, lr_t, 0.0,
                         rate_dev=torch.full((1,), rate, device="cuda"))
    assert all(_bits(x, y) for x, y in zip(got, again))


def test_clipped_ema_applies_each_segments_factor_and_follows_the_formula(case):
    """One factor per segment, the three column ranges of the fused tensor among them (pads: 1): theta, m and v are those of
    ds_adam_tf_clipped; every shadow, pads included, follows the formula from the new theta."""
    f = torch.tensor([0.9, 0.8, 0.7, 0.6, 0.5, 0.4, 0.3, 0.2, 1.0], device="cuda")
    assert case.names[2:5] == ["f0", "f1", "f2"]
    lr_t, rate = 2e-3, RATES[1]
    flags = torch.zeros(4, dtype=torch.int32, device="cuda")
    got = _clipped_ema(case, f, flags, lr_t, float(rate))
    want = case.adam_clipped(f, flags, lr_t)
    for x, y, what in zip(got, want, ("theta", "m", "v")):
        assert _bits(x, y), what
    assert _bits(got[3], E.update32(case.shadow, got[0], rate))
    err, bound = np.abs(got[3].astype(np.float64) - E.update64(case.shadow, got[0], rate)), E.bound64(case.shadow, got[0], rate)
    assert (err <= bound).all()
    assert (got[3] != case.shadow).mean() > 0.5 and flags.cpu().tolist() == [0, 0, 0, 0]


def test_clipped_ema_skips_on_the_flag_and_counts(case):
    flags = torch.tensor([1, 1, 5, 0], dtype=torch.int32, device="cuda")
    got = _clipped_ema(case, torch.full((case.nseg + 1,), 0.5, device="cuda"), flags, 1e-3, float(RATE_1))
    for x, y, what in zip(got, (case.theta, case.m, case.v, case.shadow), ("theta", "m", "v", "shadow")):
        assert _bits(x, y), what
    assert flags.cpu().tolist() == [1, 1, 6, 0]
    flags[1] = 0
    got = _clipped_ema(case, torch.full((case.nseg + 1,), 0.5, device="cuda"), flags, 1e-3, float(RATE_1))
    assert not _bits(got[0], case.theta) and not _bits(got[3], case.shadow) and flags.cpu().tolist() == [1, 0, 6, 0]


def test_bad_arguments_are_codes_before_any_launch(case):
    from tumblr_emotions_amd import _lib, ops
    c = Flat(1020, seed=1)
    theta, g, m, v, shadow = c.dev()
    flags = torch.zeros(4, dtype=torch.int32, device="cuda")
    factors = torch.ones(case.nseg + 1, device="cuda")
    for rate in (-1e-3, 1.0 + 1e-6, float("nan"), float("inf")):
        with pytest.raises(RuntimeError, match="ds_adam_tf_ema"):
            ops.adam_tf_ema(theta, g, m, v, shadow, c.n, c.n_wd, WD, SCALE, 1e-3, rate, B1, B2, EPS)
        with pytest.raises(RuntimeError, match="ds_adam_tf_clipped_ema"):
            _clipped_ema(case, factors, flags, 1e-3, rate)
    lib, p, s = _lib.load(), ops._p, ops._stream()
    assert lib.ds_adam_tf_ema(p(theta), p(g), p(m), p(v), None, c.n, c.n_wd, WD, SCALE, 1e-3, None, 0.5, None, B1, B2, EPS, s) == -1
    assert b"ds_adam_tf_ema" in lib.ds_last_error()
    assert lib.ds_adam_tf_clipped_ema(p(theta), p(g), p(m), p(v), None, c.n, c.n_wd, WD, SCALE, 1e-3, None, 0.5, None, B1, B2,
                                      EPS, p(case.seg), case.nseg, p(case.chunks), case.nchunks, p(factors), p(flags), s) == -1
    assert b"ds_adam_tf_clipped_ema" in lib.ds_last_error()
    torch.cuda.synchronize()
    for x, y in zip((theta, g, m, v, shadow), (c.theta, c.g, c.m, c.v, c.shadow)):
        assert _bits(x, y)
    assert flags.cpu().tolist() == [0, 0, 0, 0]


# =========================================================================================================================
# the training step
# =========================================================================================================================
def _batch(i, mode="text", rows=8):
    from tumblr_emotions_amd.synthetic import synthetic_batch_numpy, to_device
    return to_device(synthetic_batch_numpy(rows, 10, 50, seed=4 + i, with_images=(mode != "text")))


def _net(mode="text", **kw):
    from tumblr_emotions_amd.net import SentimentNet
    net = SentimentNet(mode=mode, **dict(TEXT, **kw))
    net.initialize(seed=3)
    return net


def _in_lockstep(mode, steps, decay, **kw):
    """A net with the key and one without, step by step: the same loss, theta, m, v (and moving statistics); the shadows are
    the fp32 recurrence on the net's own theta."""
    plain, net = _net(mode, **kw), _net(mode, moving_average_decay=decay, **kw)
    assert plain.store.ema is None and net.store.ema is not None
    assert _bits(net.store.ema, net.store.theta)                      # shadow_0 = theta_0
    ref = E.Recurrence(decay, net.store.theta.cpu().numpy())
    for i in range(steps):
        batch = _batch(i, mode)
        plain.train_step(batch, 1e-3)
        net.train_step(batch, 1e-3)
        la, lb = plain.total_loss_value(), net.total_loss_value()
        assert la == lb and math.isfinite(la), (i, la, lb)
        for name in ("theta", "m", "v", "grad", "frozen"):
            assert torch.equal(getattr(net.store, name), getattr(plain.store, name)), (name, i)
        want = ref.step(net.store.theta.cpu().numpy())
        assert _bits(net.store.ema, want), "shadows after step %d" % (i + 1)
        assert not _bits(net.store.ema, net.store.theta)
    return net


@pytest.mark.parametrize("decay", [0.5, 0.9999])
def test_text_steps_keep_adams_bits_and_the_shadows_follow_the_recurrence(decay):
    """12 steps: at decay 0.5 the min changes sides at t = 8, so both branches of the schedule are walked."""
    assert E.decay_exact(0.5, 7) < Fraction(1, 2) and E.decay_exact(0.5, 8) == Fraction(1, 2) == E.decay_exact(0.5, 12)
    net = _in_lockstep("text", 12, decay)
    assert net.step == 12


@pytest.mark.parametrize("frozen_bn", [False, True], ids=["batch_stats", "frozen_bn"])
def test_joint_steps_and_the_names_of_the_averages(frozen_bn):
    net = _in_lockstep("joint", 2, 0.9999, frozen_bn=frozen_bn)
    st = net.store
    avg = net.averages_state_dict()
    trainable = [n for e in st.entries.values() if e.trainable for n in ([c[0] for c in e.columns] if e.columns else [e.name])]
    assert sorted(avg) == sorted(trainable) and sorted(trainable) == sorted(st.clip_names)
    assert not any("moving_" in n for n in avg)                       # BatchNorm's moving statistics get no shadow
    fused = [e for e in st.entries.values() if e.trainable and e.columns and len(e.columns) == 3 and len(e.shape) == 4]
    assert len(fused) == 1 and all("Mixed_5c" in n for (n, _, _) in fused[0].columns)
    whole = st.ema[fused[0].offset:fused[0].offset + fused[0].numel].view(fused[0].shape).cpu().numpy()
    for (name, c0, c1) in fused[0].columns:
        assert avg[name].shape == fused[0].shape[:-1] + (c1 - c0,) and _bits(avg[name], np.ascontiguousarray(whole[..., c0:c1]))
    for e in st.entries.values():
        if e.trainable and not e.columns:
            assert _bits(avg[e.name], st.ema[e.offset:e.offset + e.numel].view(e.shape).cpu().numpy()), e.name
    # load_state_dict(which='ema') is the inverse
    keep = st.ema.clone()
    st.ema.zero_()
    assert net.load_averages_state_dict(avg) == set(avg)
    used = torch.zeros_like(keep, dtype=torch.bool)
    for e in st.entries.values():
        if e.trainable:
            used[e.offset:e.offset + e.numel] = True
    assert torch.equal(st.ema[used], keep[used])


def test_without_the_key_the_new_launches_are_never_made(monkeypatch):
    from tumblr_emotions_amd import ops

    def boom(*a, **k):
        raise AssertionError("a net without moving_average_decay reached the _ema launches")

    monkeypatch.setattr(ops, "adam_tf_ema", boom)
    monkeypatch.setattr(ops, "adam_tf_clipped_ema", boom)
    calls = []
    adam = ops.adam_tf
    monkeypatch.setattr(ops, "adam_tf", lambda *a, **k: (calls.append(1), adam(*a, **k))[1])
    net = _net()
    for i in range(2):
        net.train_step(_batch(i), 1e-3)
    assert len(calls) == 2 and net.store.ema is None and net.ema_rate_dev is None
    net.train_step(_batch(2), 1e-3, num_clones=2)
    batch = _batch(3)
    assert net.capture_step(batch)
    net.train_step(batch, 1e-3)
    clipped = _net(clip_global_norm=1e-2, skip_nonfinite_steps=True)
    clipped.train_step(_batch(0), 1e-3)
    torch.cuda.synchronize()
    assert clipped.store.ema is None
    for n in (net, clipped):
        with pytest.raises(RuntimeError, match="moving_average_decay"):
            n.averages_state_dict()
        with pytest.raises(RuntimeError, match="moving_average_decay"):
            with n.averaged_weights():
                pass


# ---- clones and data parallelism -----------------------------------------------------------------------------------------
DP_CLIP, DP_DECAY = 1e-2, 0.9999


def _state(net):
    torch.cuda.synchronize()
    return dict(net.state_dict(), adam_m=net.store.m.cpu().numpy(), adam_v=net.store.v.cpu().numpy(),
                ema=net.store.ema.cpu().numpy(), factor=np.float64(net.grad_norms()["factor"]))


def _dp_ema_worker(rank, world, port, out):
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    from tumblr_emotions_amd import dp
    dp.init_distributed("gloo", device=0, rank=rank, world_size=world)
    try:
        from tumblr_emotions_amd.net import SentimentNet
        from tumblr_emotions_amd.synthetic import synthetic_batch_numpy, to_device
        net = SentimentNet(mode="text", clip_global_norm=DP_CLIP, moving_average_decay=DP_DECAY, **TEXT)
        net.initialize(seed=3)
        states = []
        for i in range(2):
            local = to_device(synthetic_batch_numpy(8, 10, 50, seed=4 + i, with_images=False), "cuda", rank, world)
            net.train_step(local, 1e-3)
            states.append(_state(net))
        out.put((rank, states))
    finally:
        dist.destroy_process_group()


def test_two_clones_equal_both_ranks_of_a_two_rank_run_shadows_included():
    ctx = mp.get_context("spawn")
    out = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_dp_ema_worker, args=(r, 2, port, out)) for r in range(2)]
    for p in procs:
        p.start()
    net = _net(clip_global_norm=DP_CLIP, moving_average_decay=DP_DECAY)
    ref = E.Recurrence(DP_DECAY, net.store.theta.cpu().numpy())
    mine = []
    for i in range(2):
        net.train_step(_batch(i), 1e-3, num_clones=2)
        mine.append(_state(net))
        assert _bits(net.store.ema, ref.step(net.store.theta.cpu().numpy()))
    got = dict(_collect(out, procs, 2))
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    for i in range(2):
        assert mine[i]["factor"] < 0.5
        for theirs in (got[0], got[1]):
            assert sorted(mine[i]) == sorted(theirs[i])
            for k in mine[i]:
                assert np.array_equal(mine[i][k], theirs[i][k]), (i, k)


def test_replays_of_a_captured_step_equal_eager_steps_shadows_included():
    """Two replays against two eager steps; then the captured net validates inside averaged_weights() and its third step is
    still a replay, equal to the eager net's third step."""
    batch = _batch(0)
    outs = []
    for graphed in (False, True):
        net = _net(moving_average_decay=0.5)
        if graphed:
            start = [x.clone() for x in (net.store.theta, net.store.ema)]
            assert net.capture_step(batch)
            torch.cuda.synchronize()
            assert torch.equal(net.store.theta, start[0]) and torch.equal(net.store.ema, start[1]) and net.step == 0
        for i in range(2):
            net.train_step(batch, 1e-3 * (0.5 ** i))
        torch.cuda.synchronize()
        assert (net._graph is not None) == graphed and net.step == 2
        two = [x.clone() for x in (net.store.theta, net.store.m, net.store.v, net.store.ema)]
        if graphed:
            with net.averaged_weights():
                net.predict(batch)
            assert net._graph is not None
        net.train_step(batch, 1e-3)
        torch.cuda.synchronize()
        assert (net._graph is not None) == graphed
        outs.append(two + [x.clone() for x in (net.store.theta, net.store.m, net.store.v, net.store.ema)])
    for a, b in zip(outs[0], outs[1]):
        assert torch.equal(a, b)
    assert not torch.equal(outs[0][3], outs[0][0]) and not torch.equal(outs[0][7], outs[0][3])


def test_a_skipped_step_leaves_the_shadows_alone_but_counts():
    """The guard's skip (b_softmax = +Inf: every gradient is NaN) leaves store.ema bit for bit; the step after it is update
    t = 3 of the schedule."""
    batch = _batch(0)
    net = _net(clip_global_norm=1.0, skip_nonfinite_steps=True, moving_average_decay=0.9999)
    ref = E.Recurrence(0.9999, net.store.theta.cpu().numpy())
    net.train_step(batch, 1e-3)
    torch.cuda.synchronize()
    assert _bits(net.store.ema, ref.step(net.store.theta.cpu().numpy()))
    bias = net.store.view("b_softmax")
    keep = bias.clone()
    bias[3] = float("inf")
    before = [x.clone() for x in (net.store.theta, net.store.m, net.store.v, net.store.ema)]
    net.train_step(batch, 1e-3)
    assert net.grad_norms()["skipped_steps"] == 1 and net.step == 2
    for x, y in zip((net.store.theta, net.store.m, net.store.v, net.store.ema), before):
        assert _bits(x, y)
    ref.step(None, skipped=True)
    bias.copy_(keep)
    net.train_step(batch, 1e-3)
    torch.cuda.synchronize()
    assert ref.t == 2 and E.rate32(0.9999, 3) != E.rate32(0.9999, 2)
    assert _bits(net.store.ema, ref.step(net.store.theta.cpu().numpy()))
    assert bool(torch.isfinite(net.store.ema).all())


# ---- averaged_weights() --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["text", "joint"])
def test_averaged_weights_exchange_and_restore(mode):
    from tumblr_emotions_amd.net import SentimentNet
    a, b = (_net(mode, moving_average_decay=0.5) for _ in range(2))      # b never enters the context
    for i in range(2):
        for n in (a, b):
            n.train_step(_batch(i, mode), 1e-3)
    torch.cuda.synchronize()
    theta, ema = a.store.theta.clone(), a.store.ema.clone()
    assert not torch.equal(theta, ema)
    avg, raw = a.averages_state_dict(), a.state_dict()
    twin = SentimentNet(mode=mode, **TEXT)
    twin.load_state_dict(dict(raw, **avg))
    batch = _batch(7, mode)
    modes = (False, True) if mode == "joint" else (False,)
    raw_logits = a.predict(batch).clone()
    want = {fused: twin.predict(batch, fused=fused).clone() for fused in modes}
    assert not torch.equal(want[False], raw_logits)                    # the averages are other weights
    ptr = a.store.theta.data_ptr()
    with a.averaged_weights() as inside:
        assert inside is a and a.store.theta.data_ptr() == ptr
        assert torch.equal(a.store.theta, ema) and torch.equal(a.store.ema, theta)
        for fused in modes:
            assert _bits(a.predict(batch, fused=fused), want[fused]), fused
        if mode == "text":
            assert _bits(a.forward(batch), want[False])
        inner = a.averages_state_dict()
        assert sorted(inner) == sorted(avg) and all(_bits(inner[k], avg[k]) for k in avg)
        with pytest.raises(RuntimeError, match="averaged_weights"):
            a.train_step(batch, 1e-3)
        with pytest.raises(RuntimeError, match="averaged_weights"):
            a.train_step(batch, 1e-3, num_clones=2)
        with pytest.raises(RuntimeError, match="averaged_weights"):
            a.capture_step(batch)
        with pytest.raises(RuntimeError, match="nest"):
            with a.averaged_weights():
                pass
        assert torch.equal(a.store.theta, ema)                         # the refused calls changed nothing
    torch.cuda.synchronize()
    assert torch.equal(a.store.theta, theta) and torch.equal(a.store.ema, ema) and a.step == b.step == 2
    assert _bits(a.predict(batch), raw_logits)
    # an exception inside still exchanges back
    with pytest.raises(KeyError):
        with a.averaged_weights():
            raise KeyError("x")
    assert torch.equal(a.store.theta, theta) and torch.equal(a.store.ema, ema)
    for n in (a, b):
        n.train_step(_batch(2, mode), 1e-3)
    torch.cuda.synchronize()
    assert a.total_loss_value() == b.total_loss_value()
    for name in ("theta", "m", "v", "ema", "grad", "frozen"):
        assert torch.equal(getattr(a.store, name), getattr(b.store, name)), name


# ---- the front end ---------------------------------------------------------------------------------------------------------
def _lines(path):
    with open(path) as f:
        return [json.loads(l) for l in f if l.strip()]


def test_train_and_evaluate_text_model_with_moving_averages(tmp_path):
    from tumblr_emotions_amd.text_model.text_embedding import _CONFIG, TextModel, evaluate_text_model, train_text_model
    from tumblr_emotions_amd.training import load_checkpoint
    steps, M = 6, 2
    cfg = dict(SMALL_TEXT, moving_average_decay=0.9)
    dirs = {k: str(tmp_path / k) for k in ("valid", "plain", "nokey")}
    train_text_model(dirs["valid"], steps, config=dict(cfg, validate_every=3, validate_batches=M, keep_best=True), quiet=True)
    train_text_model(dirs["plain"], steps, config=cfg, quiet=True)
    train_text_model(dirs["nokey"], 1, config=SMALL_TEXT, quiet=True)
    lines = _lines(os.path.join(dirs["valid"], "validation.jsonl"))
    assert [l["global_step"] for l in lines] == [3, 6] and all(l["weights"] == "averaged" for l in lines)
    cks = {k: torch.load(os.path.join(d, "model.ckpt-%d.pt" % (1 if k == "nokey" else steps)), map_location="cpu",
                         weights_only=True) for k, d in dirs.items()}
    assert "moving_averages" not in cks["nokey"]
    a, b = cks["valid"], cks["plain"]
    trainable = sorted(n for n in a["variables"] if n != "Text/W_embedding")
    assert sorted(a["moving_averages"]) == trainable
    # validation changes nothing: variables, Adam slots and shadows of the run without validate_every, bit for bit
    for group in ("variables", "moving_averages"):
        assert sorted(a[group]) == sorted(b[group])
        for k in a[group]:
            assert _bits(a[group][k], b[group][k]), (group, k)
    assert _bits(a["adam_m"], b["adam_m"]) and _bits(a["adam_v"], b["adam_v"])
    assert any(not _bits(a["moving_averages"][k], a["variables"][k]) for k in trainable)
    best = torch.load(os.path.join(dirs["valid"], "model.best.pt"), map_location="cpu", weights_only=True)
    assert sorted(best["moving_averages"]) == trainable and sorted(best["variables"]) == sorted(a["variables"])
    # load_checkpoint restores the shadows; averaged=True loads them in place of the variables
    model = TextModel(dict(_CONFIG, **cfg))
    path = os.path.join(dirs["valid"], "model.ckpt-%d.pt" % steps)
    assert load_checkpoint(model, path) == steps
    net = model.net
    got = net.averages_state_dict()
    assert all(_bits(got[k], a["moving_averages"][k]) for k in trainable)
    assert all(_bits(net.state_dict()[k], a["variables"][k]) for k in a["variables"])
    batches = [model.next_batch(10 ** 6 + i) for i in range(M)]
    correct = total = 0
    with net.averaged_weights():
        for batch in batches:
            correct += int((net.predict(batch).argmax(dim=1) == batch["labels"]).sum().item())
            total += int(batch["labels"].shape[0])
        inside = [net.predict(batch).clone() for batch in batches]
    acc = evaluate_text_model(dirs["valid"], str(tmp_path / "log"), "validation", M, config=cfg, quiet=True)
    assert acc == correct / total and acc == lines[-1]["accuracy"]
    other = TextModel(dict(_CONFIG, **cfg))
    load_checkpoint(other, path, averaged=True)
    sd = other.net.state_dict()
    assert all(_bits(sd[k], a["moving_averages"][k]) for k in trainable)
    assert _bits(sd["Text/W_embedding"], a["variables"]["Text/W_embedding"])
    assert _bits(other.net.store.ema, other.net.store.theta)
    for batch, want in zip(batches, inside):
        assert _bits(other.net.predict(batch), want)
    # a net without the key restores the variables of such a file and ignores its averages
    plain_model = TextModel(dict(_CONFIG, **SMALL_TEXT))
    load_checkpoint(plain_model, path)
    assert plain_model.net.store.ema is None
    assert all(_bits(plain_model.net.state_dict()[k], a["variables"][k]) for k in a["variables"])
    # a file without averages: the shadows start at the variables; asking for the averages is a KeyError
    load_checkpoint(model, os.path.join(dirs["nokey"], "model.ckpt-1.pt"))
    assert _bits(model.net.store.ema, model.net.store.theta)
    with pytest.raises(KeyError, match="moving_average_decay"):
        evaluate_text_model(dirs["nokey"], str(tmp_path / "log2"), "validation", M, config=cfg, quiet=True)
    with pytest.raises(ValueError, match="moving_average_decay"):
        train_text_model(str(tmp_path / "bad"), 1, config=dict(cfg, moving_average_decay=1.0), quiet=True)


def test_joint_and_image_front_ends_take_the_key(tmp_path):
    """train_deep_sentiment with frozen_bn, fused_inference and validate_every=1, train_image_model plain: validation runs
    on the averages and changes no bit of the run; the last validation line is what evaluate_* reports with the key."""
    from tumblr_emotions_amd.image_model.im_model import evaluate_image_model, train_image_model
    from tumblr_emotions_amd.image_text_model.im_text_rnn_model import evaluate_deep_sentiment, train_deep_sentiment
    cfg = dict(SMALL_TEXT, batch_size=4, num_samples=8, frozen_bn=True, fused_inference=True, moving_average_decay=0.5)
    dirs = [str(tmp_path / n) for n in ("plain", "valid", "image")]
    train_deep_sentiment(None, dirs[0], 2, config=cfg, quiet=True)
    train_deep_sentiment(None, dirs[1], 2, config=dict(cfg, validate_every=1, validate_batches=2), quiet=True)
    a, b = (torch.load(os.path.join(d, "model.ckpt-2.pt"), map_location="cpu", weights_only=True) for d in dirs[:2])
    for group in ("variables", "moving_averages"):
        assert sorted(a[group]) == sorted(b[group])
        assert all(_bits(a[group][k], b[group][k]) for k in a[group]), group
    assert _bits(a["adam_m"], b["adam_m"]) and _bits(a["adam_v"], b["adam_v"])
    assert not any("moving_" in k for k in a["moving_averages"]) and any(k.endswith("moving_mean") for k in a["variables"])
    assert any(not _bits(a["moving_averages"][k], a["variables"][k]) for k in a["moving_averages"])
    lines = _lines(os.path.join(dirs[1], "validation.jsonl"))
    assert [l["global_step"] for l in lines] == [1, 2] and all(l["weights"] == "averaged" for l in lines)
    acc = evaluate_deep_sentiment(dirs[1], str(tmp_path / "log"), "validation", 2, config=dict(cfg, eval_metrics=True), quiet=True)
    (line,) = _lines(tmp_path / "log" / "validation" / "metrics.jsonl")
    assert line["confusion"] == lines[-1]["confusion"] and line["loss"] == lines[-1]["loss"] and acc == lines[-1]["accuracy"]
    # without the key the same checkpoint is scored on its variables: another loss
    evaluate_deep_sentiment(dirs[1], str(tmp_path / "raw"), "validation", 2,
                            config=dict({k: v for k, v in cfg.items() if k != "moving_average_decay"}, eval_metrics=True), quiet=True)
    (raw,) = _lines(tmp_path / "raw" / "validation" / "metrics.jsonl")
    assert raw["loss"] != line["loss"]
    icfg = dict(batch_size=4, num_samples=8, synthetic=True, moving_average_decay=0.5)
    train_image_model(None, dirs[2], 2, config=dict(icfg, validate_every=1, validate_batches=1), quiet=True)
    ilines = _lines(os.path.join(dirs[2], "validation.jsonl"))
    assert [l["global_step"] for l in ilines] == [1, 2] and all(l["weights"] == "averaged" for l in ilines)
    acc = evaluate_image_model(dirs[2], str(tmp_path / "ilog"), "validation", 1, config=dict(icfg, eval_metrics=True), quiet=True)
    (iline,) = _lines(tmp_path / "ilog" / "validation" / "metrics.jsonl")
    assert iline["confusion"] == ilines[-1]["confusion"] and iline["loss"] == ilines[-1]["loss"] and acc == ilines[-1]["accuracy"]
