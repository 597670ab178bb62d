"""Gradient clipping and the non-finite step guard on the GPU: ds_grad_norms and ds_adam_tf_clipped against
fp64 NumPy on a hand-made layout, then the training step against the fp64 oracle.  The oracle has no clipping: the tests
apply TensorFlow's definitions (tests/grad_clip_ref.py) to its gradients and step with S.adam_step.

Adam's first step from zero slots is almost invariant to the scale of the gradient, so the step tests gate the SLOTS m and v
after the first step, and theta after a second step from non-zero slots."""
import json
import math
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from oracle import tf_semantics as S
from oracle import torch_ref as R

import grad_clip_ref as G
from test_dp_gpu import JOINT, TEXT, _collect, _dp_parity_inputs, _free_port
from test_model_gpu import _dev_batch, _grad_close

pytestmark = pytest.mark.gpu

B1, B2, EPS = 0.9, 0.999, 1e-8
DBL_MAX = 1.7976931348623157e308


# =========================================================================================================================
# the kernels
# =========================================================================================================================
WD, SCALE = 0.25, 0.5          # (a weight decay large enough for the L2 term to matter in the sums)
GUARD = 8                      # canary elements on either side of every output


class Case:
    """Segments of 1, 3 (padded to 4), 4096 (one chunk exactly), 4097 (a chunk of one element) and 2^20 + 4 elements (257
    chunks) and a 5 x 12 tensor split into the columns 0:5, 5:6, 6:12.  ParamStore lays the L2 part out first, so n_wd =
    4 + 4 + 60 + 4096 ends between `c` and `d`.  Pad elements hold non-zero values everywhere: no sum may count them, and
    the optimiser must treat them as ds_adam_tf does."""

    def __init__(self, seed=0):
        from tumblr_emotions_amd.params import ParamStore
        st = ParamStore(device="cuda")
        st.declare("a", (1,), True, l2=True)
        st.declare("b", (3,), True, l2=True)
        st.declare("fused", (1, 1, 5, 12), True, l2=True, columns=[("f0", 0, 5), ("f1", 5, 6), ("f2", 6, 12)])
        st.declare("c", (4096,), True, l2=True)
        st.declare("d", (4097,), True)
        st.declare("e", ((1 << 20) + 4,), True)
        st.finalize()
        self.st, self.n, self.n_wd = st, st.theta.numel(), st.n_l2
        assert self.n_wd == 4 + 4 + 60 + 4096 and self.n == self.n_wd + 4100 + (1 << 20) + 4
        self.names = st.clip_names
        assert self.names == ["a", "b", "f0", "f1", "f2", "c", "d", "e"]
        self.seg, self.chunks = st.clip_tables()
        self.nseg, self.nchunks = self.seg.shape[0], self.chunks.shape[0]
        assert self.nchunks == 1 + 1 + 3 + 1 + 2 + 257 + 3      # + the three pad chunks behind a, b and d
        rng = np.random.RandomState(seed)
        self.theta = rng.standard_normal(self.n).astype(np.float32)
        self.g = (rng.standard_normal(self.n) * 10.0 ** rng.uniform(-3, 1, size=self.n)).astype(np.float32)
        self.m = (0.1 * rng.standard_normal(self.n)).astype(np.float32)
        self.v = (0.01 * rng.uniform(0.1, 1, size=self.n)).astype(np.float32)
        self.idx = [G.flat_indices(row, 0, int(row[1] * row[4])) for row in st.clip_segments]
        self.owner = np.full(self.n, -1)
        for s, i in enumerate(self.idx):
            self.owner[i] = s

    def g_eff64(self, g=None):
        g = self.g if g is None else g
        ge = g.astype(np.float64) * SCALE
        ge[:self.n_wd] += WD * self.theta[:self.n_wd].astype(np.float64)
        return ge

    def outputs(self):
        """(partials, sumsq, factors, flags) as views inside canaried buffers; partials start as NaN."""
        bufs = []
        for count, dtype, fill in ((self.nchunks, torch.float64, float("nan")), (self.nseg + 1, torch.float64, -3.0),
                                   (self.nseg + 1, torch.float32, -3.0), (4, torch.int32, 0)):
            whole = torch.full((count + 2 * GUARD,), 77, dtype=dtype, device="cuda")
            whole[GUARD:GUARD + count] = fill
            bufs.append(whole)
        return bufs, [w[GUARD:w.numel() - GUARD] for w in bufs]

    @staticmethod
    def canaries_intact(bufs):
        return all(bool((w[:GUARD] == 77).all()) and bool((w[-GUARD:] == 77).all()) for w in bufs)

    def norms(self, mode, clip, guard, g=None, flags_init=(0, 0, 0, 0)):
        from tumblr_emotions_amd import ops
        bufs, (partials, sumsq, factors, flags) = self.outputs()
        flags.copy_(torch.tensor(flags_init, dtype=torch.int32))
        theta, gd = torch.from_numpy(self.theta).cuda(), torch.from_numpy(self.g if g is None else g).cuda()
        ops.grad_norms(theta, gd, self.n, self.n_wd, WD, SCALE, self.seg, self.chunks, mode, clip, guard, partials, sumsq,
                       factors, flags)
        torch.cuda.synchronize()
        assert self.canaries_intact(bufs)
        assert np.array_equal(theta.cpu().numpy(), self.theta) and np.array_equal(gd.cpu().numpy(), self.g if g is None else g,
                                                                                   equal_nan=True)      # inputs are only read
        return partials, sumsq, factors, flags

    def state(self):
        return [torch.from_numpy(x.copy()).cuda() for x in (self.theta, self.m, self.v)]

    def adam_clipped(self, factors, flags, lr_t, g=None, lr_t_dev=None):
        from tumblr_emotions_amd import ops
        theta, m, v = self.state()
        gd = torch.from_numpy(self.g if g is None else g).cuda()
        ops.adam_tf_clipped(theta, gd, m, v, self.n, self.n_wd, WD, SCALE, lr_t, B1, B2, EPS, self.seg, self.chunks, factors, flags,
                            lr_t_dev=lr_t_dev)
        torch.cuda.synchronize()
        return [x.cpu().numpy() for x in (theta, m, v)]


@pytest.fixture(scope="module")
def case():
    return Case()


def _expected_factor(sumsq, c):
    if not abs(sumsq) <= DBL_MAX:
        return np.float32("nan")
    return np.float32(c / max(math.sqrt(sumsq), c))


def test_sums_against_fp64_and_bit_reproducible(case):
    """Per-segment and global sums of g_eff^2 against fp64 NumPy.  The kernel squares and adds in double, so what it loses
    is the fp32 rounding of each g_eff = fl(fl(g s) + fl(wd w)): at most 2 u (|g s| + |wd w|) with u = 2^-24 (two roundings
    of terms bounded by the sum of magnitudes), i.e. a relative 4 u = 2.4e-7 of sum (|g s| + |wd w|)^2 on the squares --
    gated at 1e-6 of it, the 8 x 1.2e-7 of the all-positive bound.  Every partial of the NaN-filled workspace is written;
    pad chunks give 0; two runs leave the same bits."""
    from tumblr_emotions_amd import ops
    runs = [case.norms(ops.CLIP_NONE, 0.0, False) for _ in range(2)]
    partials, sumsq, factors, flags = (x.cpu().numpy() for x in runs[0])
    for a, b in zip(runs[0], runs[1]):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    assert np.isfinite(partials).all()
    pad = case.st.clip_chunks[:, 0] == -1
    assert (partials[pad] == 0.0).all() and (partials[~pad] > 0.0).all()
    ge = case.g_eff64()
    mag = np.abs(case.g.astype(np.float64) * SCALE)
    mag[:case.n_wd] += np.abs(WD * case.theta[:case.n_wd].astype(np.float64))
    want, bound = np.zeros(case.nseg + 1), np.zeros(case.nseg + 1)
    for s, i in enumerate(case.idx):
        want[s], bound[s] = np.sum(ge[i] ** 2), 1e-6 * np.sum(mag[i] ** 2)
    want[-1], bound[-1] = want[:-1].sum(), bound[:-1].sum()
    err = np.abs(sumsq - want)
    print("sum of squares, error / bound per segment and global:", np.round(err / bound, 4))
    assert (err <= bound).all(), (err / bound)
    # (a sum that counted a pad element, or missed the L2 term, is off by far more: pads hold N(0, 1) values)
    assert (factors == 1.0).all() and flags.tolist() == [0, 0, 0, 0]


def test_factors_follow_the_formula_on_the_kernels_own_sums(case):
    from tumblr_emotions_amd import ops
    _, sumsq, _, _ = case.norms(ops.CLIP_NONE, 0.0, False)
    sumsq = sumsq.cpu().numpy()
    nrm = np.sqrt(sumsq)
    c_mid = float(np.sqrt(nrm[2] * nrm[5]))      # between two segments' norms: some clip, some do not
    for mode, c in ((ops.CLIP_PER_VARIABLE, c_mid), (ops.CLIP_GLOBAL, c_mid), (ops.CLIP_GLOBAL, 0.37 * float(nrm[-1])),
                    (ops.CLIP_PER_VARIABLE, float(nrm[:-1].max())),      # AT the largest norm: nothing clips
                    (ops.CLIP_PER_VARIABLE, 2.0 * float(nrm[:-1].max())),
                    (ops.CLIP_GLOBAL, float(nrm[-1])), (ops.CLIP_GLOBAL, 1e30)):
        _, sumsq2, factors, flags = case.norms(mode, c, True)
        assert sumsq2.cpu().numpy().tobytes() == sumsq.tobytes()
        f = factors.cpu().numpy()
        if mode == ops.CLIP_PER_VARIABLE:
            want = np.array([_expected_factor(x, c) for x in sumsq[:-1]] + [np.float32(1.0)])
        else:
            want = np.full(case.nseg + 1, _expected_factor(sumsq[-1], c))
        assert f.tobytes() == want.tobytes(), (mode, c, f, want)
        assert flags.cpu().tolist() == [0, 0, 0, 0]
        if c >= (nrm[:-1].max() if mode == ops.CLIP_PER_VARIABLE else nrm[-1]):
            assert (f == np.float32(1.0)).all(), (mode, c, f)
        else:
            assert (f < 1.0).any()
    f = case.norms(ops.CLIP_PER_VARIABLE, c_mid, False)[2].cpu().numpy()
    assert (f[:-1] < 1.0).sum() >= 2 and (f[:-1] == 1.0).sum() >= 2


def test_optimiser_with_unit_factors_has_the_bits_of_adam_tf(case):
    """Every factor 1.0f, no skip: theta, m and v of ds_adam_tf on the same buffers, pads included; lr_t from the host
    and from device memory."""
    from tumblr_emotions_amd import ops
    _, _, factors, flags = case.norms(ops.CLIP_GLOBAL, 1e30, True)
    for lr_t, on_device in ((3e-3, False), (7e-4, True)):
        lr_dev = torch.full((1,), lr_t, device="cuda") if on_device else None
        got = case.adam_clipped(factors, flags, 1e3 if on_device else lr_t, lr_t_dev=lr_dev)
        theta, m, v = case.state()
        ops.adam_tf(theta, torch.from_numpy(case.g).cuda(), m, v, case.n, case.n_wd, WD, SCALE, 1e3 if on_device else lr_t,
                    B1, B2, EPS, lr_t_dev=lr_dev)
        torch.cuda.synchronize()
        for x, y, what in zip(got, (theta, m, v), ("theta", "m", "v")):
            assert x.tobytes() == y.cpu().numpy().tobytes(), what
        assert not np.array_equal(got[0], case.theta)
    assert flags.cpu().tolist() == [0, 0, 0, 0]


def test_optimiser_applies_each_segments_factor(case):
    """Distinct factors per segment (pads: 1) against S.adam_step in fp64 on g_eff * factor, at the project's gate for one
    Adam step: 1e-5 on the resolved entries (here: all of them -- both sides start from the same fp32 state); m and v to
    1e-5 of their largest entry.  The fp64 step takes beta1, beta2 and epsilon as the fp32 values the kernel receives:
    1 - fl(0.999) is 1.3e-5 away from 0.001 in relative terms, which is ds_adam_tf's arithmetic too (tests/head_ref.py adam_ref)
    and would otherwise be all of v's error."""
    t, lr = 3, 1e-3
    lr_t = lr * math.sqrt(1 - B2 ** t) / (1 - B1 ** t)
    f = np.array([0.9, 0.8, 0.7, 0.6, 0.5, 0.4, 0.3, 0.2, 1.0], np.float32)
    flags = torch.zeros(4, dtype=torch.int32, device="cuda")
    theta, m, v = case.adam_clipped(torch.from_numpy(f).cuda(), flags, lr_t)
    per_elem = np.where(case.owner >= 0, f[case.owner].astype(np.float64), 1.0)
    w64, m64, v64 = S.adam_step(case.theta.astype(np.float64), case.g_eff64() * per_elem, case.m.astype(np.float64),
                                case.v.astype(np.float64), t, lr, b1=float(np.float32(B1)), b2=float(np.float32(B2)),
                                eps=float(np.float32(EPS)))
    assert np.abs(theta - w64).max() <= 1e-5
    assert np.abs(m - m64).max() <= 1e-5 * np.abs(m64).max() and np.abs(v - v64).max() <= 1e-5 * np.abs(v64).max()
    # ... and each segment really got ITS factor: with the neighbour's factor the slots miss the gate
    for s in range(case.nseg - 1):
        i = case.idx[s]
        other = case.g_eff64()[i] * float(f[s + 1])
        m_other = B1 * case.m[i] + (1 - B1) * other
        assert np.abs(m[i] - m_other).max() > 1e-5 * np.abs(m64).max() or len(i) < 4, case.names[s]
    assert flags.cpu().tolist() == [0, 0, 0, 0]


def test_optimiser_skips_on_the_flag_and_counts(case):
    flags = torch.tensor([1, 1, 5, 0], dtype=torch.int32, device="cuda")
    factors = torch.full((case.nseg + 1,), 0.5, device="cuda")
    got = case.adam_clipped(factors, flags, 1e-3)
    for x, y in zip(got, (case.theta, case.m, case.v)):
        assert x.tobytes() == y.tobytes()
    assert flags.cpu().tolist() == [1, 1, 6, 0]
    flags[1] = 0                                   # non-finite reported but no guard: the step is taken, nothing is counted
    got = case.adam_clipped(factors, flags, 1e-3)
    assert not np.array_equal(got[0], case.theta) and flags.cpu().tolist() == [1, 0, 6, 0]


def test_non_finite_gradients_with_and_without_the_guard(case):
    """One NaN in `c` and one +Inf in `e`.  Guard on: the step is skipped.  Guard off, per variable: those two variables turn
    NaN (a NaN factor, as tf.clip_by_norm gives), the others take the step they take on the clean gradient.  Guard off,
    global: every variable turns NaN, as tf.clip_by_global_norm documents."""
    from tumblr_emotions_amd import ops
    g = case.g.copy()
    ic, ie = case.names.index("c"), case.names.index("e")
    g[case.idx[ic][17]] = np.nan
    g[case.idx[ie][(1 << 20) + 1]] = np.inf
    clean_sums = case.norms(ops.CLIP_NONE, 0.0, False)[1].cpu().numpy()
    c = 0.5 * float(np.sqrt(clean_sums[:-1].min()))            # every variable clips
    _, _, f_clean, flags_clean = case.norms(ops.CLIP_PER_VARIABLE, c, False)
    clean = case.adam_clipped(f_clean, flags_clean, 1e-3)
    bad = np.zeros(case.nseg, bool)
    bad[[ic, ie]] = True
    # guard on
    _, sumsq, factors, flags = case.norms(ops.CLIP_PER_VARIABLE, c, True, g=g, flags_init=(0, 0, 2, 0))
    sumsq = sumsq.cpu().numpy()
    assert np.isnan(sumsq[ic]) and np.isinf(sumsq[ie]) and np.isfinite(sumsq[:-1][~bad]).all() and not np.isfinite(sumsq[-1])
    assert np.array_equal(sumsq[:-1][~bad], clean_sums[:-1][~bad])
    assert flags.cpu().tolist() == [1, 1, 2, 0]
    got = case.adam_clipped(factors, flags, 1e-3, g=g)
    for x, y in zip(got, (case.theta, case.m, case.v)):
        assert x.tobytes() == y.tobytes()
    assert flags.cpu().tolist() == [1, 1, 3, 0]
    # guard off, per variable
    _, _, factors, flags = case.norms(ops.CLIP_PER_VARIABLE, c, False, g=g)
    f = factors.cpu().numpy()
    assert np.isnan(f[:-1][bad]).all() and np.array_equal(f[:-1][~bad], f_clean.cpu().numpy()[:-1][~bad])
    assert flags.cpu().tolist() == [1, 0, 0, 0]
    got = case.adam_clipped(factors, flags, 1e-3, g=g)
    for s in range(case.nseg):
        for x, y in zip(got, clean):
            if bad[s]:
                assert np.isnan(x[case.idx[s]]).all(), case.names[s]
            else:
                assert x[case.idx[s]].tobytes() == y[case.idx[s]].tobytes(), case.names[s]
    for x, y in zip(got, clean):
        assert x[case.owner < 0].tobytes() == y[case.owner < 0].tobytes()      # pads: factor 1, finite
    # guard off, global
    _, _, factors, flags = case.norms(ops.CLIP_GLOBAL, c, False, g=g)
    assert np.isnan(factors.cpu().numpy()).all() and flags.cpu().tolist() == [1, 0, 0, 0]
    got = case.adam_clipped(factors, flags, 1e-3, g=g)
    for x in got:
        assert np.isnan(x[case.owner >= 0]).all() and np.isfinite(x[case.owner < 0]).all()


def test_bad_arguments_are_codes_before_any_launch(case):
    from tumblr_emotions_amd import ops
    bufs, (partials, sumsq, factors, flags) = case.outputs()
    theta = torch.zeros(case.n, device="cuda")
    for mode, c in ((ops.CLIP_GLOBAL, 0.0), (ops.CLIP_PER_VARIABLE, -1.0), (ops.CLIP_GLOBAL, float("nan")),
                    (ops.CLIP_GLOBAL, float("inf")), (3, 1.0)):
        with pytest.raises(RuntimeError, match="ds_grad_norms"):
            ops.grad_norms(theta, theta, case.n, case.n_wd, WD, SCALE, case.seg, case.chunks, mode, c, False, partials, sumsq,
                           factors, flags)
    torch.cuda.synchronize()
    assert bool(torch.isnan(partials).all())


# =========================================================================================================================
# the training step
# =========================================================================================================================
V, D, H, T = 40, 12, 16, 9            # the dims of test_clones_gpu
SMALL = dict(nb_emotions=15, rnn_size=H, vocab_size=V, embedding_dim=D, post_size=T)


def _text_problem(B, seed):
    rng = np.random.RandomState(seed)
    params = R.make_params("text", rng, num_classes=15, embed_dim=D, rnn_size=H, dtype=np.float64)
    params["Text/rnn/basic_lstm_cell/bias"] = rng.normal(0, 0.1, size=4 * H)
    emb = S.synthetic_embedding(V, D).astype(np.float64)
    batch = S.synthetic_batch(B, T, V, seed=seed + 1, with_images=False)
    return params, emb, batch


def _slots(net, names):
    torch.cuda.synchronize()
    out = {}
    for which in ("m", "v"):
        buf = getattr(net.store, which)
        for name, row in zip(net.store.clip_names, net.store.clip_segments):
            if name in names:
                out[which, name] = buf[torch.from_numpy(G.flat_indices(row, 0, int(row[1] * row[4]))).to(buf.device)].cpu().numpy()
    return out


def _norms_close(gn, per, glob, tol=1e-3):
    """grad_norms() against the oracle at the gradient gate: 1e-3 relative."""
    for name, x in per.items():
        assert abs(gn[name] - x) <= tol * x, (name, gn[name], x)
    assert abs(gn["global_norm"] - glob) <= tol * glob


def _check_slots(net, g, f, m_prev=None, v_prev=None):
    """m = b1 m' + (1 - b1) f g and v = b2 v' + (1 - b2) (f g)^2 at the gradient gate 1e-3 (relative L2 and max-norm); for v,
    whose new term is the square, the relative error of the gradient doubles: 2e-3."""
    got = _slots(net, set(g))
    for name in g:
        gc = np.asarray(g[name], np.float64).ravel() * f[name]
        m0 = 0.0 if m_prev is None else m_prev[name].ravel()
        v0 = 0.0 if v_prev is None else v_prev[name].ravel()
        _grad_close(got["m", name], B1 * m0 + (1 - B1) * gc, "m of " + name, 1e-3)
        _grad_close(got["v", name], B2 * v0 + (1 - B2) * gc * gc, "v of " + name, 2e-3)


def test_text_steps_with_global_clipping_follow_the_clipped_oracle():
    """Step 1 clips at half the oracle's global norm (factor 0.5); step 2, from the clipped state with non-zero slots, runs with
    a threshold of twice its norm: only the not-clipping regime.  lr = 1e-2: on the oracle alone the clipped and the
    unclipped run then sit more than 10 x the 1e-5 gate apart after step 2 (at 1e-3 they would not: Adam normalises most of
    a gradient's scale away), so the test can tell them apart."""
    from tumblr_emotions_amd.net import SentimentNet
    lr, B = 1e-2, 8
    params, emb, batch = _text_problem(B, 31)
    batch["seq_lens"][0], batch["seq_lens"][1] = 1, T
    batch["texts"][0, 1:] = V
    batch2 = S.synthetic_batch(B, T, V, seed=77, with_images=False)
    ref = R.DeepSentimentRef(params, emb, "text", torch.float64)
    names = list(ref.trainable)
    g1 = {n: g.numpy() for n, g in ref.train_step(batch, lr)["grads"].items()}
    per1, glob1 = G.norms(g1)
    c1 = 0.5 * glob1
    w = {n: np.asarray(params[n], np.float64).copy() for n in names}
    m = {n: np.zeros_like(w[n]) for n in names}
    v = {n: np.zeros_like(w[n]) for n in names}
    wu, mu, vu = ({n: x[n].copy() for n in names} for x in (w, m, v))      # the unclipped run, same gradients
    f1 = G.clipped_adam_step(S, w, g1, m, v, 1, lr, "global", c1)
    G.clipped_adam_step(S, wu, g1, mu, vu, 1, lr, None, None)
    assert all(abs(x - 0.5) < 1e-12 for x in f1.values())

    net = SentimentNet(mode="text", clip_global_norm=c1, **SMALL)
    net.load_state_dict(dict(params, **{"Text/W_embedding": emb}))
    net.train_step(_dev_batch(batch), lr)
    gn = net.grad_norms()
    _norms_close(gn, per1, glob1)
    assert abs(gn["factor"] - 0.5) <= 1e-3 and not gn["nonfinite"] and gn["skipped_steps"] == 0 and "factors" not in gn
    assert set(gn) == set(names) | {"global_norm", "factor", "nonfinite", "skipped_steps"}
    _check_slots(net, g1, f1)
    # grads_state_dict() keeps returning the unclipped sum
    grads = net.grads_state_dict()
    for n in names:
        _grad_close(grads[n], g1[n], "gradient of " + n, 1e-3)

    # step 2 from the clipped fp64 state
    ref2 = R.DeepSentimentRef(dict(params, **w), emb, "text", torch.float64)
    g2 = {n: g.numpy() for n, g in ref2.train_step(batch2, lr)["grads"].items()}
    per2, glob2 = G.norms(g2)
    c2 = 2.0 * glob2
    m1, v1 = {n: m[n].copy() for n in names}, {n: v[n].copy() for n in names}
    net.load_state_dict(dict(params, **dict(w, **{"Text/W_embedding": emb})))
    net.store.load_state_dict(m1, which="m")
    net.store.load_state_dict(v1, which="v")
    assert net.step == 1
    f2 = G.clipped_adam_step(S, w, g2, m, v, 2, lr, "global", c2)
    G.clipped_adam_step(S, wu, g2, mu, vu, 2, lr, None, None)
    assert all(x == 1.0 for x in f2.values())
    assert max(np.abs(w[n] - wu[n]).max() for n in names) > 10 * 1e-5      # (on the oracle alone)
    net.clip_norm = c2
    net.train_step(_dev_batch(batch2), lr)
    gn = net.grad_norms()
    _norms_close(gn, per2, glob2)
    assert gn["factor"] == 1.0 and net.step == 2
    _check_slots(net, g2, f2, m1, v1)
    after = net.state_dict()
    for n in names:
        d = np.abs(after[n].reshape(w[n].shape) - w[n])
        assert d.max() <= 2.5 * lr + 1e-6, n
        big = np.abs(g2[n]) > 1e-2 * max(np.abs(g2[n]).max(), 1e-12)
        assert (d[big] <= 1e-5).mean() >= 0.99, "%s: %.4f of the resolved entries within 1e-5 (worst %.3e)" % (
            n, (d[big] <= 1e-5).mean(), d[big].max())


def test_joint_step_clips_each_variable_by_its_own_norm():
    """B = 4 (the first rows of test_dp_gpu's parity inputs, dropout off).  A guard-only net takes the step first: its
    forward pass gives the ReLU / pool decisions the fp64 oracle follows (test_model_gpu._check_step explains why) and its
    grad_norms() the unclipped norms.  The threshold is the median of the oracle's 71 per-variable norms -- which IS one
    variable's norm, so it is moved to the geometric mean of that norm and the next larger one: 'no norm within 1 % of the
    threshold' is then a condition on the inputs, checked below with the other two.  The clipping net then takes the same
    step (same bits up to the optimiser) and its m slots must be 0.1 x factor x gradient, variable by variable -- the three
    block-input 1x1 convs of Mixed_5c, which share one fused tensor, each by its own factor."""
    from hip_decisions import hip_decisions, keep_activations
    from tumblr_emotions_amd.net import SentimentNet
    params, emb, batch = _dp_parity_inputs()
    batch = {k: np.ascontiguousarray(v[:4]) for k, v in batch.items()}
    dev = _dev_batch(batch)
    lr = 1e-3

    def fresh(**kw):
        net = SentimentNet(mode="joint", dropout_keep_prob=1.0, **dict(JOINT, **kw))
        net.load_state_dict(dict(params, **{"Text/W_embedding": emb}))
        keep_activations(net)      # (both nets: the same launches, so the same gradient bits)
        return net

    plain = fresh(skip_nonfinite_steps=True)
    plain.train_step(dev, lr)
    torch.cuda.synchronize()
    ref = R.DeepSentimentRef(params, emb, "joint", torch.float64)
    ref.inject = hip_decisions(plain)
    g = {n: x.numpy() for n, x in ref.train_step(batch, lr)["grads"].items()}
    assert len(g) == 71
    per, glob = G.norms(g)
    gn0 = plain.grad_norms()
    _norms_close(gn0, per, glob)
    assert all(x == 1.0 for x in gn0["factors"].values()) and set(gn0["factors"]) == set(g)
    ordered = sorted(per.values())
    c = math.sqrt(ordered[35] * ordered[36])
    clip = [n for n, x in per.items() if x > c]
    assert len(clip) >= 3 and len(per) - len(clip) >= 3 and all(abs(x - c) > 0.01 * c for x in per.values())
    f = G.factors(g, "variable", c)

    net = fresh(clip_gradient_norm=c)
    net.train_step(dev, lr)
    gn = net.grad_norms()
    for n in g:
        assert gn[n] == gn0[n], n                    # the same gradient buffer, the same reduction: the same bits
        assert abs(gn["factors"][n] - f[n]) <= 1e-3 * f[n], (n, gn["factors"][n], f[n])
        assert (gn["factors"][n] == 1.0) == (n not in clip), n
    assert "factor" not in gn and not gn["nonfinite"]
    _check_slots(net, g, f)
    fused = [e for e in net.store.entries.values() if e.trainable and e.columns and len(e.columns) == 3 and len(e.shape) == 4]
    assert len(fused) == 1
    three = [n for (n, _, _) in fused[0].columns]
    assert len({round(per[n], 12) for n in three}) == 3 and len({gn[n] for n in three}) == 3
    print("Mixed_5c block-input variables: norms %s, factors %s" % ([per[n] for n in three], [f[n] for n in three]))
    # their slots carry their OWN factor: with another variable's clipped factor the m slot misses the gate
    got = _slots(net, set(three))
    for n in three:
        others = [f[x] for x in clip if abs(f[x] - f[n]) > 0.01 * f[n]]
        want = 0.1 * g[n].ravel() * f[n]
        for fo in others[:3]:
            assert np.linalg.norm(got["m", n] - want * fo / f[n]) > 1e-3 * np.linalg.norm(want), n
    # the variables that did not clip took the plain net's step, bit for bit
    a, b = net.state_dict(), plain.state_dict()
    for n in g:
        if n not in clip:
            assert np.array_equal(a[n], b[n]), n
    assert torch.equal(net.store.grad, plain.store.grad)


def _run(mode, steps, dtype="f32", rows=8, **kw):
    from tumblr_emotions_amd.net import SentimentNet
    from tumblr_emotions_amd.synthetic import synthetic_batch_numpy, to_device
    net = SentimentNet(mode=mode, dtype=dtype, **dict(TEXT, **kw))
    net.initialize(seed=3)
    losses = []
    for i in range(steps):
        net.train_step(to_device(synthetic_batch_numpy(rows, 10, 50, seed=4 + i, with_images=(mode != "text"))), 1e-3)
        losses.append(net.total_loss_value())
    torch.cuda.synchronize()
    return net, losses


@pytest.mark.parametrize("mode, dtype, steps", [("text", "f32", 2), ("joint", "f32", 2), ("joint", "bf16", 1)])
def test_a_threshold_nothing_reaches_changes_no_bit(mode, dtype, steps):
    """Threshold 1e30 plus the guard on finite gradients: every factor is exactly 1.0f and the shared per-element update
    gives ds_adam_tf's bits -- theta, m, v and the loss of the plain net."""
    plain, l0 = _run(mode, steps, dtype)
    for kw in (dict(clip_global_norm=1e30, skip_nonfinite_steps=True), dict(clip_gradient_norm=1e30, skip_nonfinite_steps=True)):
        net, l1 = _run(mode, steps, dtype, **kw)
        assert l0 == l1 and all(x == x for x in l0)
        for name in ("theta", "m", "v", "grad", "frozen"):
            assert torch.equal(getattr(net.store, name), getattr(plain.store, name)), name
        gn = net.grad_norms()
        assert gn["skipped_steps"] == 0 and not gn["nonfinite"] and gn["global_norm"] > 0


def test_without_the_keys_the_new_launches_are_never_made(monkeypatch):
    from tumblr_emotions_amd import ops

    def boom(*a, **k):
        raise AssertionError("a net without the clipping keys reached the clipping launches")

    monkeypatch.setattr(ops, "grad_norms", boom)
    monkeypatch.setattr(ops, "adam_tf_clipped", boom)
    calls = []
    adam = ops.adam_tf
    monkeypatch.setattr(ops, "adam_tf", lambda *a, **k: (calls.append(1), adam(*a, **k))[1])
    net, _ = _run("text", 2)
    assert len(calls) == 2 and net.clip_state is None
    net2, _ = _run("text", 1, rows=8)
    from tumblr_emotions_amd.synthetic import synthetic_batch_numpy, to_device
    net2.train_step(to_device(synthetic_batch_numpy(8, 10, 50, seed=9, with_images=False)), 1e-3, num_clones=2)
    batch = to_device(synthetic_batch_numpy(8, 10, 50, seed=9, with_images=False))
    assert net2.capture_step(batch)
    net2.train_step(batch, 1e-3)
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match="grad_norms"):
        net2.grad_norms()


# ---- clones and data parallelism -----------------------------------------------------------------------------------------
DP_CLIP = 1e-2          # far below the text model's gradient norm at initialisation: every step clips (asserted)


def _state(net):
    torch.cuda.synchronize()
    return dict(net.state_dict(), adam_m=net.store.m.cpu().numpy(), adam_v=net.store.v.cpu().numpy(),
                factor=np.float64(net.grad_norms()["factor"]))


def _dp_clip_worker(rank, world, port, out):
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    from tumblr_emotions_amd import dp
    dp.init_distributed("gloo", device=0, rank=rank, world_size=world)
    try:
        from tumblr_emotions_amd.net import SentimentNet
        from tumblr_emotions_amd.synthetic import synthetic_batch_numpy, to_device
        net = SentimentNet(mode="text", clip_global_norm=DP_CLIP, **TEXT)
        net.initialize(seed=3)
        states = []
        for i in range(2):
            local = to_device(synthetic_batch_numpy(8, 10, 50, seed=4 + i, with_images=False), "cuda", rank, world)
            net.train_step(local, 1e-3)
            states.append(_state(net))
        out.put((rank, states))
    finally:
        dist.destroy_process_group()


def test_clipped_two_clones_equal_both_ranks_of_a_two_rank_run_bit_for_bit():
    """Text, clip_global_norm: one process with K = 2 on 8 rows against two gloo ranks of 4 rows (test_dp_gpu's harness).
    Every rank reduces the same summed buffer with the same kernels: the ranks equal each other and the clone run."""
    from tumblr_emotions_amd.net import SentimentNet
    from tumblr_emotions_amd.synthetic import synthetic_batch_numpy, to_device
    ctx = mp.get_context("spawn")
    out = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_dp_clip_worker, args=(r, 2, port, out)) for r in range(2)]
    for p in procs:
        p.start()
    net = SentimentNet(mode="text", clip_global_norm=DP_CLIP, **TEXT)
    net.initialize(seed=3)
    mine = []
    for i in range(2):
        net.train_step(to_device(synthetic_batch_numpy(8, 10, 50, seed=4 + i, with_images=False)), 1e-3, num_clones=2)
        mine.append(_state(net))
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


def test_two_replays_of_a_captured_clipped_step_equal_two_eager_steps():
    from tumblr_emotions_amd.net import SentimentNet
    from tumblr_emotions_amd.synthetic import synthetic_batch_numpy, to_device
    batch = to_device(synthetic_batch_numpy(8, 10, 50, seed=1, with_images=False))
    outs = []
    for graphed in (False, True):
        net = SentimentNet(mode="text", clip_global_norm=DP_CLIP, skip_nonfinite_steps=True, **TEXT)
        net.initialize(seed=3)
        if graphed:
            assert net.capture_step(batch)
        for i in range(2):
            net.train_step(batch, 1e-3 * (0.5 ** i))
        torch.cuda.synchronize()
        assert (net._graph is not None) == graphed and net.step == 2
        gn = net.grad_norms()
        assert gn["factor"] < 0.5 and gn["skipped_steps"] == 0
        outs.append((net.store.theta.clone(), net.store.m.clone(), net.store.v.clone(), gn))
    for a, b in zip(outs[0][:3], outs[1][:3]):
        assert torch.equal(a, b)
    assert outs[0][3] == outs[1][3]


def test_a_non_finite_step_is_skipped_and_the_next_one_is_step_two():
    """b_softmax of one class is +Inf: the logits of that class are +Inf, so the loss and every gradient are NaN.  (The text
    tower's persistent kernels poll ticket counters and placement words, csrc/lstm_seq.hip wait_counter / group_on_one_xcd,
    both bounded: no loop bound or poll there reads a data value, so non-finite data cannot stall them.)  The guard leaves
    theta, m and v untouched bit for bit and counts one skipped step; `step` still advances, so after the bias is restored
    the next step is the step a net takes with step == 2 from the same state."""
    from tumblr_emotions_amd.net import SentimentNet
    from tumblr_emotions_amd.synthetic import synthetic_batch_numpy, to_device
    batch = to_device(synthetic_batch_numpy(8, 10, 50, seed=2, with_images=False))
    net = SentimentNet(mode="text", clip_global_norm=1.0, skip_nonfinite_steps=True, **TEXT)
    net.initialize(seed=3)
    net.train_step(batch, 1e-3)                      # a finite step first: non-zero slots
    torch.cuda.synchronize()
    bias = net.store.view("b_softmax")
    keep = bias.clone()
    bias[3] = float("inf")
    before = [x.clone() for x in (net.store.theta, net.store.m, net.store.v)]
    net.train_step(batch, 1e-3)
    gn = net.grad_norms()
    assert gn["nonfinite"] and gn["skipped_steps"] == 1 and net.step == 2
    assert not math.isfinite(gn["global_norm"]) and math.isnan(net.total_loss_value())
    assert not any(math.isfinite(gn[n]) for n in net.store.clip_names)
    for x, y in zip((net.store.theta, net.store.m, net.store.v), before):
        assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()
    bias.copy_(keep)
    twin = SentimentNet(mode="text", clip_global_norm=1.0, **TEXT)      # the same clipping, no guard, at the same state
    for name in ("theta", "m", "v", "frozen"):
        getattr(twin.store, name).copy_(getattr(net.store, name))
    twin.after_load()
    twin.step = 2
    net.train_step(batch, 1e-3)
    twin.train_step(batch, 1e-3)
    torch.cuda.synchronize()
    assert net.step == twin.step == 3
    gn = net.grad_norms()
    assert not gn["nonfinite"] and gn["skipped_steps"] == 1 and 0.0 < gn["factor"] <= 1.0
    for name in ("theta", "m", "v"):
        assert torch.equal(getattr(net.store, name), getattr(twin.store, name)), name
    assert bool(torch.isfinite(net.store.theta).all())


def test_train_text_model_clips_and_logs_gradient_norms(tmp_path):
    from tumblr_emotions_amd.text_model.text_embedding import _CONFIG, TextModel, train_text_model
    cfg = dict(synthetic=True, batch_size=4, num_samples=24, initial_lr=1e-3, rnn_size=32, vocab_size=60, embedding_dim=20,
               post_size=12, clip_global_norm=DP_CLIP, log_gradient_norms=True)
    d = str(tmp_path / "clip")
    train_text_model(d, 12, config=cfg, quiet=True)
    with open(os.path.join(d, "gradients.jsonl")) as f:
        lines = [json.loads(l) for l in f if l.strip()]
    assert [l["global_step"] for l in lines] == [10, 12]          # run_training's logging steps
    names = TextModel(dict(_CONFIG, **cfg)).net.store.tf_names()
    trainable = [n for n in names if n != "Text/W_embedding"]
    for l in lines:
        assert sorted(l["norms"]) == sorted(trainable) and all(x > 0 for x in l["norms"].values())
        assert abs(l["global_norm"] - math.sqrt(sum(x * x for x in l["norms"].values()))) <= 1e-9 * l["global_norm"]
        assert abs(l["factor"] - DP_CLIP / l["global_norm"]) <= 1e-6 * l["factor"] and l["skipped_steps"] == 0
        assert l["nonfinite"] is False
    with pytest.raises(ValueError, match="log_gradient_norms"):
        train_text_model(str(tmp_path / "none"), 1, config=dict(cfg, clip_global_norm=None), quiet=True)
    with pytest.raises(ValueError, match="mutually exclusive"):
        train_text_model(str(tmp_path / "both"), 1, config=dict(cfg, clip_gradient_norm=1.0), quiet=True)
