"""slim's optimiser choice on the GPU: ds_opt_step against the four Adam entry points (bit for bit) and
against the fp32 / fp64 restatements of TF's updates (tests/optim_ref.py), then the training step with every option that
surrounds the optimiser, and the text front end with a learning-rate schedule and a resumed run.  [TF-sem]: the updates are
TF's restated, parity unpinned."""
import json
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import ema_ref as E
import optim_ref as O
from test_dp_gpu import TEXT, _collect, _free_port
from test_ema_gpu import Flat, _batch, _bits, _magnitudes, _net
from test_frontends_gpu import SMALL_TEXT
from test_grad_clip_gpu import Case

pytestmark = pytest.mark.gpu

B1, B2, EPS = 0.9, 0.999, 1e-8
MU, RHO = 0.9, 0.9
WD, SCALE = 0.25, 0.5
GRID_PASS = 2048 * 256            # elements of one grid-stride pass: stream_grid caps the grid at 8 blocks per CU
SIZES = (4, 1020, 1028, GRID_PASS + 260)
KINDS = ("sgd", "momentum", "rmsprop")
RATE = E.rate32(0.9999, 1)
# sqrtf and / of the build (no fast-math flag) are correctly rounded: rmsprop's mom and theta are the restatement's bits too.
# Were they not, the fp64 bound alone would gate them (it is asserted either way).
RMSPROP_BITS = True


def _hyper(kind, eps=1.0):
    return {"adam": dict(b1=B1, b2=B2, eps=EPS), "sgd": {}, "momentum": dict(momentum=MU),
            "rmsprop": dict(momentum=MU, rho=RHO, eps=eps)}[kind]


def _step(kind, bufs, n, n_wd, lr, eps=1.0, **kw):
    """One ds_opt_step on device buffers (theta, g, slot0, slot1[, ...]); returns theta, slot0, slot1 as arrays."""
    from tumblr_emotions_amd import ops
    theta, g, s0, s1 = bufs[:4]
    ops.opt_step(ops.OPT_KINDS[kind], theta, g, s0, s1, n, n_wd, WD, SCALE, lr, **dict(_hyper(kind, eps), **kw))
    torch.cuda.synchronize()
    return [x.cpu().numpy() for x in (theta, s0, s1)]


def _ref32(kind, theta, s0, s1, gi, lr, eps=1.0, hyper=None):
    """(theta', slot0', slot1') of the fp32 restatement; a slot the kind does not own comes back as it went in."""
    h = hyper or {"momentum": MU, "rmsprop_decay": RHO, "opt_epsilon": eps, "adam_beta1": B1, "adam_beta2": B2}
    if kind == "sgd":
        return O.sgd32(theta, gi, lr), s0, s1
    if kind == "momentum":
        w, a = O.momentum32(theta, s0, gi, lr, h["momentum"])
        return w, a, s1
    if kind == "rmsprop":
        return O.rmsprop32(theta, s0, s1, gi, lr, h["momentum"], h["rmsprop_decay"], h["opt_epsilon"])
    return O.adam32(theta, s0, s1, gi, lr, h["adam_beta1"], h["adam_beta2"], h["opt_epsilon"])


def _check(kind, got, theta, s0, s1, gi, lr, eps=1.0, hyper=None, what=""):
    """got = (theta', slot0', slot1') of the device against the restatements: bits wherever +, -, * are the only operations
    (sgd, momentum, rmsprop's ms); rmsprop's mom and theta inside the fp64 bound, and the restatement's bits as well."""
    want = _ref32(kind, theta, s0, s1, gi, lr, eps, hyper)
    if kind != "rmsprop":
        for x, y, name in zip(got, want, ("theta", "slot0", "slot1")):
            assert _bits(x, y), (kind, name, what)
        return 0.0
    h = hyper or {"momentum": MU, "rmsprop_decay": RHO, "opt_epsilon": eps}
    assert _bits(got[2], want[2]), ("rmsprop", "ms", what)
    qw, qmom, _ = O.rmsprop64(theta, s0, s1, gi, lr, h["momentum"], h["rmsprop_decay"], h["opt_epsilon"])
    worst = max(O.worst_ratio(got[0], qw), O.worst_ratio(got[1], qmom))
    assert worst <= 1.0, ("rmsprop", what, worst)
    if RMSPROP_BITS:
        assert _bits(got[1], want[1]) and _bits(got[0], want[0]), ("rmsprop", "mom / theta", what)
    return worst


# =========================================================================================================================
# the kernels
# =========================================================================================================================
@pytest.mark.parametrize("n", SIZES)
def test_adam_kind_has_the_bits_of_adam_tf_and_adam_tf_ema(n):
    from tumblr_emotions_amd import ops
    c = Flat(n, seed=n % 1000)
    lr_t = 3e-3
    a = c.dev()
    ops.adam_tf(a[0], a[1], a[2], a[3], n, c.n_wd, WD, SCALE, lr_t, B1, B2, EPS)
    b = c.dev()
    got = _step("adam", b, n, c.n_wd, lr_t)
    assert all(_bits(x, y) for x, y in zip(got, (a[0], a[2], a[3]))) and not _bits(got[0], c.theta)
    assert _bits(b[1], c.g) and _bits(b[4], c.shadow)
    a = c.dev()
    ops.adam_tf_ema(a[0], a[1], a[2], a[3], a[4], n, c.n_wd, WD, SCALE, lr_t, float(RATE), B1, B2, EPS)
    b = c.dev()
    got = _step("adam", b, n, c.n_wd, lr_t, shadow=b[4], ema_rate=float(RATE))
    assert all(_bits(x, y) for x, y in zip(got, (a[0], a[2], a[3]))) and _bits(b[4], a[4]) and not _bits(b[4], c.shadow)


@pytest.fixture(scope="module")
def case():
    c = Case()
    c.shadow = _magnitudes(np.random.RandomState(5), c.n)
    return c


def _case_bufs(case):
    theta, m, v = case.state()
    return [theta, torch.from_numpy(case.g).cuda(), m, v, torch.from_numpy(case.shadow.copy()).cuda()]


def _clip_kw(case, factors, flags):
    return dict(segments=case.seg, chunks=case.chunks, factors=factors, flags=flags)


def test_adam_kind_has_the_bits_of_adam_tf_clipped_and_clipped_ema(case):
    from tumblr_emotions_amd import ops
    f = torch.tensor([0.9, 0.8, 0.7, 0.6, 0.5, 0.4, 0.3, 0.2, 1.0], device="cuda")
    lr_t = 2e-3
    flags = torch.zeros(4, dtype=torch.int32, device="cuda")
    want = case.adam_clipped(f, flags, lr_t)
    b = _case_bufs(case)
    got = _step("adam", b, case.n, case.n_wd, lr_t, **_clip_kw(case, f, flags))
    assert all(_bits(x, y) for x, y in zip(got, want)) and _bits(b[4], case.shadow) and not _bits(got[0], case.theta)
    a = _case_bufs(case)
    ops.adam_tf_clipped_ema(a[0], a[1], a[2], a[3], a[4], case.n, case.n_wd, WD, SCALE, lr_t, float(RATE), B1, B2, EPS, case.seg,
                            case.chunks, f, flags)
    b = _case_bufs(case)
    got = _step("adam", b, case.n, case.n_wd, lr_t, shadow=b[4], ema_rate=float(RATE), **_clip_kw(case, f, flags))
    assert all(_bits(x, y) for x, y in zip(got, (a[0], a[2], a[3]))) and _bits(b[4], a[4]) and not _bits(b[4], case.shadow)
    assert flags.cpu().tolist() == [0, 0, 0, 0]


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", ["sgd", "momentum"])
def test_sgd_and_momentum_are_the_fp32_restatement(kind, n):
    c = Flat(n, seed=n % 1000)
    gi = O.g_eff32(c.theta, c.g, c.n_wd, WD, SCALE)
    for lr in (3e-3, 0.5):
        b = c.dev()
        got = _step(kind, b, n, c.n_wd, lr)
        _check(kind, got, c.theta, c.m, c.v, gi, lr)
        assert _bits(b[1], c.g) and not _bits(got[0], c.theta)                # g is never written
        assert _bits(got[2], c.v) and (kind == "momentum") != _bits(got[1], c.m)      # sgd leaves both slots, momentum slot1
    # sgd reads no slot: NULL slots are fine
    from tumblr_emotions_amd import ops
    if kind == "sgd":
        b = c.dev()
        ops.opt_step(ops.OPT_SGD, b[0], b[1], None, None, n, c.n_wd, WD, SCALE, 3e-3)
        torch.cuda.synchronize()
        assert _bits(b[0], O.sgd32(c.theta, gi, 3e-3))


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("eps", [1.0, 1e-10])
def test_rmsprop_ms_is_the_fp32_restatement_and_mom_theta_lie_inside_the_fp64_bound(eps, n):
    c = Flat(n, seed=n % 1000)
    gi = O.g_eff32(c.theta, c.g, c.n_wd, WD, SCALE)
    worst = 0.0
    for lr in (3e-3, 0.5):
        b = c.dev()
        got = _step("rmsprop", b, n, c.n_wd, lr, eps=eps)
        want = _ref32("rmsprop", c.theta, c.m, c.v, gi, lr, eps)
        print("n = %d eps = %g lr = %g: mom bits %s, theta bits %s" % (n, eps, lr, _bits(got[1], want[1]), _bits(got[0], want[0])))
        worst = max(worst, _check("rmsprop", got, c.theta, c.m, c.v, gi, lr, eps))
        assert _bits(b[1], c.g) and (got[2] > 0).all() and not _bits(got[0], c.theta) and not _bits(got[1], c.m)
    print("n = %d eps = %g: largest |error| / bound against fp64 = %.5f" % (n, eps, worst))


@pytest.mark.parametrize("kind", KINDS)
def test_averages_ride_behind_every_kind(kind):
    """With a shadow: theta and slots are the bits of the call without one, the shadow is TF's update on the new theta."""
    for n in SIZES:
        c = Flat(n, seed=n % 1000)
        plain = _step(kind, c.dev(), n, c.n_wd, 3e-3)
        for rate in (RATE, np.float32(0.01), np.float32(0.0)):
            b = c.dev()
            got = _step(kind, b, n, c.n_wd, 3e-3, shadow=b[4], ema_rate=float(rate))
            assert all(_bits(x, y) for x, y in zip(got, plain)), (n, float(rate))
            assert _bits(b[4], E.update32(c.shadow, got[0], rate)) and _bits(b[1], c.g)
            assert _bits(b[4], c.shadow) == (rate == 0)


@pytest.mark.parametrize("kind", KINDS)
def test_clipped_form_unit_factors_segment_factors_and_the_skip_flag(kind, case):
    from tumblr_emotions_amd import ops
    lr = 2e-3
    flags = torch.zeros(4, dtype=torch.int32, device="cuda")
    # every factor 1.0: the bits of the unclipped call (pads included)
    plain = _step(kind, _case_bufs(case), case.n, case.n_wd, lr)
    got = _step(kind, _case_bufs(case), case.n, case.n_wd, lr, **_clip_kw(case, torch.ones(case.nseg + 1, device="cuda"), flags))
    assert all(_bits(x, y) for x, y in zip(got, plain))
    # factors below 1, one per variable (tf.clip_by_norm) and one for all (tf.clip_by_global_norm): the reference on
    # gi * factor; pad elements have factor 1; the shadow follows the new theta
    per_variable = np.array([0.9, 0.8, 0.7, 0.6, 0.5, 0.4, 0.3, 0.2, 1.0], np.float32)
    for f in (per_variable, np.full(case.nseg + 1, 0.37, np.float32)):
        each = np.where(case.owner >= 0, f[np.maximum(case.owner, 0)], np.float32(1.0)).astype(np.float32)
        gi = O.g_eff32(case.theta, case.g, case.n_wd, WD, SCALE, each)
        b = _case_bufs(case)
        got = _step(kind, b, case.n, case.n_wd, lr, shadow=b[4], ema_rate=float(RATE),
                    **_clip_kw(case, torch.from_numpy(f).cuda(), flags))
        _check(kind, got, case.theta, case.m, case.v, gi, lr, what="factors %g.." % f[0])
        assert _bits(b[4], E.update32(case.shadow, got[0], RATE)) and _bits(b[1], case.g)
        assert not all(_bits(x, y) for x, y in zip(got, plain))
    assert flags.cpu().tolist() == [0, 0, 0, 0]
    # flags[1] set: nothing changes but flags[2]
    flags = torch.tensor([1, 1, 5, 0], dtype=torch.int32, device="cuda")
    b = _case_bufs(case)
    got = _step(kind, b, case.n, case.n_wd, lr, shadow=b[4], ema_rate=float(RATE),
                **_clip_kw(case, torch.full((case.nseg + 1,), 0.5, device="cuda"), flags))
    for x, y, name in zip(got + [b[4], b[1]], (case.theta, case.m, case.v, case.shadow, case.g), ("theta", "slot0", "slot1", "shadow", "g")):
        assert _bits(x, y), name
    assert flags.cpu().tolist() == [1, 1, 6, 0]
    # a clipped descriptor without factors is an error code (RuntimeError through the wrapper), before any launch
    with pytest.raises(RuntimeError, match="ds_opt_step"):
        ops.opt_step(ops.OPT_KINDS[kind], b[0], b[1], b[2], b[3], case.n, case.n_wd, WD, SCALE, lr, segments=case.seg,
                     chunks=case.chunks, flags=flags, **_hyper(kind))
    torch.cuda.synchronize()
    assert _bits(b[0], case.theta) and flags.cpu().tolist() == [1, 1, 6, 0]


@pytest.mark.parametrize("kind", KINDS)
def test_device_scalars_override_the_descriptors(kind, case):
    n = 1028
    c = Flat(n, seed=28)
    lr = 3e-3
    b = c.dev()
    want = _step(kind, b, n, c.n_wd, lr, shadow=b[4], ema_rate=float(RATE))
    d = c.dev()
    got = _step(kind, d, n, c.n_wd, 1e3, shadow=d[4], ema_rate=0.0, lr_dev=torch.full((1,), lr, device="cuda"),
                ema_rate_dev=torch.full((1,), float(RATE), device="cuda"))
    assert all(_bits(x, y) for x, y in zip(got, want)) and _bits(d[4], b[4]) and not _bits(d[4], c.shadow)
    # ... and in the clipped form
    flags = torch.zeros(4, dtype=torch.int32, device="cuda")
    f = torch.full((case.nseg + 1,), 0.37, device="cuda")
    b = _case_bufs(case)
    want = _step(kind, b, case.n, case.n_wd, lr, shadow=b[4], ema_rate=float(RATE), **_clip_kw(case, f, flags))
    d = _case_bufs(case)
    got = _step(kind, d, case.n, case.n_wd, 1e3, shadow=d[4], ema_rate=0.0, lr_dev=torch.full((1,), lr, device="cuda"),
                ema_rate_dev=torch.full((1,), float(RATE), device="cuda"), **_clip_kw(case, f, flags))
    assert all(_bits(x, y) for x, y in zip(got, want)) and _bits(d[4], b[4])


# =========================================================================================================================
# the training step
# =========================================================================================================================
LRS = (1e-2, 5e-3, 2.5e-3)


def _slots(net):
    torch.cuda.synchronize()
    st = net.store
    return [x.cpu().numpy().copy() for x in (st.theta, st.m, st.v)]


def _follows_the_reference(kind, mode="text", steps=3, clones=1, **kw):
    """A net of `kind` beside an adam net with the same seed: the same gradient after step 1, and after every step the
    reference update applied to the net's OWN store.grad and previous state (the clipping factor read from the net)."""
    from tumblr_emotions_amd.engine_image import WEIGHT_DECAY
    adam, net = _net(mode, **kw), _net(mode, optimizer=kind, **kw)
    assert net.optimizer == kind and adam.optimizer == "adam" and torch.equal(net.store.theta, adam.store.theta)
    st = net.store
    n = st.n_trainable_padded
    assert float(st.v[0]) == (1.0 if kind == "rmsprop" else 0.0) and float(st.m.abs().max()) == 0.0
    ck = {} if clones == 1 else {"num_clones": clones}
    ref = E.Recurrence(kw["moving_average_decay"], st.theta.cpu().numpy()) if "moving_average_decay" in kw else None
    for i in range(steps):
        batch = _batch(i, mode, rows=8)
        theta, s0, s1 = _slots(net)
        if i == 0:
            adam.train_step(batch, LRS[i], **ck)
        net.train_step(batch, LRS[i], **ck)
        got = _slots(net)
        if i == 0:
            assert torch.equal(net.store.grad, adam.store.grad) and net.total_loss_value() == adam.total_loss_value()
            assert not torch.equal(net.store.theta, adam.store.theta)
        factor = None
        if net.clip_active:
            factor = np.float32(net.grad_norms()["factor"])
            assert factor < 1
        gi = O.g_eff32(theta[:n], st.grad.cpu().numpy()[:n], st.n_l2, WEIGHT_DECAY, 1.0 / clones, factor)
        _check(kind, [x[:n] for x in got], theta[:n], s0[:n], s1[:n], gi, LRS[i], hyper=net.opt, what="step %d" % (i + 1))
        assert not _bits(got[0], theta)
        if ref is not None:
            assert _bits(st.ema, ref.step(got[0])) and not _bits(st.ema, st.theta)
    assert net.step == steps
    return net


@pytest.mark.parametrize("kind", KINDS)
def test_text_steps_same_gradient_and_the_reference_update(kind):
    _follows_the_reference(kind)


@pytest.mark.parametrize("kind", KINDS)
def test_text_steps_with_global_norm_clipping(kind):
    _follows_the_reference(kind, clip_global_norm=1e-2)


@pytest.mark.parametrize("kind", KINDS)
def test_text_steps_with_moving_averages(kind):
    _follows_the_reference(kind, moving_average_decay=0.5)


@pytest.mark.parametrize("kind", KINDS)
def test_text_steps_of_two_clones(kind):
    _follows_the_reference(kind, clones=2)


def test_one_small_joint_step_of_rmsprop_with_slims_epsilon():
    net = _follows_the_reference("rmsprop", mode="joint", steps=1)
    assert net.opt == {"optimizer": "rmsprop", "opt_epsilon": 1.0, "momentum": 0.9, "rmsprop_decay": 0.9}


def test_adam_with_its_own_betas_goes_through_ds_opt_step_and_default_adam_does_not(monkeypatch):
    from tumblr_emotions_amd import ops
    calls = []
    step = ops.opt_step
    monkeypatch.setattr(ops, "opt_step", lambda *a, **k: (calls.append(a[0]), step(*a, **k))[1])
    plain, explicit = _net(), _net(optimizer="adam", opt_epsilon=1e-8, adam_beta1=0.9, adam_beta2=0.999)
    for net in (plain, explicit):
        net.train_step(_batch(0), 1e-3)
    assert calls == [] and torch.equal(plain.store.theta, explicit.store.theta)
    own = _net(adam_beta1=0.5, adam_beta2=0.99, opt_epsilon=1e-3)
    theta, m, v = _slots(own)
    own.train_step(_batch(0), 1e-3)
    assert calls == [ops.OPT_ADAM]
    st = own.store
    n = st.n_trainable_padded
    from tumblr_emotions_amd.engine_image import WEIGHT_DECAY
    gi = O.g_eff32(theta[:n], st.grad.cpu().numpy()[:n], st.n_l2, WEIGHT_DECAY, 1.0)
    lr_t = 1e-3 * np.sqrt(1.0 - 0.99) / (1.0 - 0.5)
    got = _slots(own)
    want = O.adam32(theta[:n], m[:n], v[:n], gi, lr_t, 0.5, 0.99, 1e-3)
    assert _bits(got[1][:n], want[1]) and _bits(got[2][:n], want[2])      # m and v: products and sums only
    qw, _, _ = O.adam64(theta[:n], m[:n], v[:n], gi, lr_t, 0.5, 0.99, 1e-3)
    assert O.worst_ratio(got[0][:n], qw) <= 1.0


def test_three_replays_of_a_captured_rmsprop_step_equal_three_eager_steps():
    batch = _batch(0)
    outs = []
    for graphed in (False, True):
        net = _net(optimizer="rmsprop", opt_epsilon=1e-3, moving_average_decay=0.5)
        if graphed:
            start = _slots(net) + [net.store.ema.cpu().numpy()]
            assert net.capture_step(batch)
            after = _slots(net) + [net.store.ema.cpu().numpy()]
            assert all(_bits(a, b) for a, b in zip(start, after)) and net.step == 0      # the warm-up's snapshot restores
            assert float(net.store.v[0]) == 1.0
        for i in range(3):
            net.train_step(batch, LRS[i])
        assert (net._graph is not None) == graphed and net.step == 3
        outs.append(_slots(net) + [net.store.ema.cpu().numpy()])
    for a, b, what in zip(outs[0], outs[1], ("theta", "mom", "ms", "ema")):
        assert _bits(a, b), what
    assert not _bits(outs[0][3], outs[0][0])


def _dp_opt_worker(rank, world, port, out, kind):
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    from tumblr_emotions_amd import dp
    dp.init_distributed("gloo", device=0, rank=rank, world_size=world)
    try:
        from tumblr_emotions_amd.net import SentimentNet
        from tumblr_emotions_amd.synthetic import synthetic_batch_numpy, to_device
        net = SentimentNet(mode="text", optimizer=kind, clip_global_norm=1e-2, **TEXT)
        net.initialize(seed=3)
        for i in range(2):
            local = to_device(synthetic_batch_numpy(8, 10, 50, seed=4 + i, with_images=False), "cuda", rank, world)
            net.train_step(local, LRS[i])
        torch.cuda.synchronize()
        out.put((rank, [x.cpu().numpy() for x in (net.store.theta, net.store.m, net.store.v)]))
    finally:
        dist.destroy_process_group()


def test_two_ranks_end_with_identical_theta_and_slots():
    """rmsprop under data parallelism: both ranks, and a two-clone run of one process, end on the same bits."""
    ctx = mp.get_context("spawn")
    out = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_dp_opt_worker, args=(r, 2, port, out, "rmsprop")) for r in range(2)]
    for p in procs:
        p.start()
    net = _net(optimizer="rmsprop", clip_global_norm=1e-2)
    for i in range(2):
        net.train_step(_batch(i), LRS[i], num_clones=2)
    mine = _slots(net)
    got = dict(_collect(out, procs, 2))
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    for a, b, c, what in zip(got[0], got[1], mine, ("theta", "mom", "ms")):
        assert np.array_equal(a, b) and np.array_equal(a, c), what
    assert not np.array_equal(mine[1], np.zeros_like(mine[1]))


def test_a_nonfinite_gradient_leaves_momentums_accumulator_and_theta_alone():
    batch = _batch(0)
    net = _net(optimizer="momentum", skip_nonfinite_steps=True)
    net.train_step(batch, 1e-2)
    bias = net.store.view("b_softmax")
    keep = bias.clone()
    bias[3] = float("inf")                      # every gradient of the next step is NaN
    before = _slots(net)
    net.train_step(batch, 1e-2)
    assert net.grad_norms()["skipped_steps"] == 1 and net.grad_norms()["nonfinite"] and net.step == 2
    assert all(_bits(x, y) for x, y in zip(_slots(net), before))
    bias.copy_(keep)
    net.train_step(batch, 1e-2)
    after = _slots(net)
    assert net.grad_norms()["skipped_steps"] == 1 and not _bits(after[0], before[0]) and not _bits(after[1], before[1])
    assert np.isfinite(after[0]).all() and np.isfinite(after[1]).all()


# ---- the front end -------------------------------------------------------------------------------------------------------
def _lines(path):
    with open(path) as f:
        return [json.loads(l) for l in f if l.strip()]


def _load(path):
    return torch.load(path, map_location="cpu", weights_only=True)


def test_train_resume_and_evaluate_text_model_with_rmsprop_and_a_schedule(tmp_path):
    from tumblr_emotions_amd.text_model.text_embedding import _CONFIG, evaluate_text_model, train_text_model
    steps, cut = 7, 4
    cfg = dict(SMALL_TEXT, optimizer="rmsprop", opt_epsilon=1e-3, initial_lr=1e-2, learning_rate_decay_type="exponential",
               learning_rate_decay_factor=0.5, num_epochs_per_decay=1.0)
    full = dict(_CONFIG, **cfg)
    assert O.decay_steps(full, 24) == 3                      # 24 samples / 8 per batch * 1 epoch
    dirs = {k: str(tmp_path / k) for k in ("whole", "first", "second", "bad")}
    train_text_model(dirs["whole"], steps, config=cfg, quiet=True)
    # the learning rates handed to the optimiser follow the reference schedule: two halvings in seven steps
    lines = _lines(os.path.join(dirs["whole"], "learning_rate.jsonl"))
    assert [l["global_step"] for l in lines] == list(range(steps))
    want = [float(O.schedule32(full, 24, t)) for t in range(steps)]
    assert [l["learning_rate"] for l in lines] == want
    assert want[0] == want[2] == float(np.float32(1e-2)) and want[3] == want[5] == want[0] / 2 and want[6] == want[0] / 4
    whole = _load(os.path.join(dirs["whole"], "model.ckpt-%d.pt" % steps))
    assert whole["optimizer"] == {"optimizer": "rmsprop", "opt_epsilon": 1e-3, "momentum": 0.9, "rmsprop_decay": 0.9}
    assert float(whole["adam_v"].min()) > 0 and float(whole["adam_m"].abs().max()) > 0 and whole["global_step"] == steps
    # a resumed run continues bit for bit, schedule included
    train_text_model(dirs["first"], cut, config=cfg, quiet=True)
    path = os.path.join(dirs["first"], "model.ckpt-%d.pt" % cut)
    train_text_model(dirs["second"], steps, config=dict(cfg, resume_from=path), quiet=True)
    resumed = _load(os.path.join(dirs["second"], "model.ckpt-%d.pt" % steps))
    assert [l["global_step"] for l in _lines(os.path.join(dirs["second"], "learning_rate.jsonl"))] == list(range(cut, steps))
    assert [l["learning_rate"] for l in _lines(os.path.join(dirs["second"], "learning_rate.jsonl"))] == want[cut:]
    assert sorted(resumed["variables"]) == sorted(whole["variables"]) and resumed["global_step"] == steps
    for k in whole["variables"]:
        assert _bits(resumed["variables"][k], whole["variables"][k]), k
    assert _bits(resumed["adam_m"], whole["adam_m"]) and _bits(resumed["adam_v"], whole["adam_v"])
    assert resumed["optimizer"] == whole["optimizer"]
    # another kind cannot resume from it: its slots mean something else
    with pytest.raises(ValueError, match="rmsprop.*momentum"):
        train_text_model(dirs["bad"], steps, config=dict({k: v for k, v in cfg.items() if k != "opt_epsilon"},
                                                         optimizer="momentum", resume_from=path), quiet=True)
    with pytest.raises(ValueError, match="rmsprop.*adam"):
        train_text_model(dirs["bad"], steps, config=dict(SMALL_TEXT, resume_from=path), quiet=True)
    # evaluation reads variables: it takes the checkpoint whatever the keys say, and an adam run writes no 'optimizer'
    acc = evaluate_text_model(dirs["whole"], str(tmp_path / "log"), "validation", 2, config=cfg, quiet=True)
    assert 0.0 <= acc <= 1.0
    assert acc == evaluate_text_model(dirs["whole"], str(tmp_path / "log2"), "validation", 2, config=SMALL_TEXT, quiet=True)
    train_text_model(dirs["bad"], 1, config=SMALL_TEXT, quiet=True)
    assert "optimizer" not in _load(os.path.join(dirs["bad"], "model.ckpt-1.pt"))
    assert not os.path.exists(os.path.join(dirs["bad"], "learning_rate.jsonl"))
