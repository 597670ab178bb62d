"""The fp64 reference and the input builders of tests/test_bn_bwd_gpu.py, checked on their own (no GPU): the reference is the
oracle's and torch autograd's BatchNorm + ReLU backward, a plain fp32 evaluation stays inside the bounds the GPU file applies,
the exact inputs are exact, and the knife-edge inputs sit where the fused and the unfused fp32 predicate disagree."""
import numpy as np
import pytest
import torch

import bn_bwd_ref as B
from oracle import tf_semantics as S

F32 = np.float32


@pytest.mark.parametrize("M,C", [(3, 16), (1000, 12), (37, 1024)])
def test_reference_is_the_oracles_and_autograds_backward(M, C):
    b = B.build_real(M, C, seed=5, nudge=False)
    z, dy, beta = b.z.astype(np.float64), b.dy.astype(np.float64), b.beta
    y, mean, var, xhat, rstd = S.batch_norm_train(z, beta)
    # the statistics in full precision here: the reference then IS the analytic gradient
    ref = B.reference(z, dy, mean, rstd, beta - mean * rstd)
    g = dy * (y > 0)
    dz, dbeta = S.batch_norm_train_bwd(g, xhat, rstd)
    scale = np.abs(dz).max()
    assert np.abs(ref.dz - dz).max() <= 1e-12 * scale
    assert np.abs(ref.dbeta - dbeta).max() <= 1e-12 * np.abs(dbeta).max()
    zt = torch.tensor(z, requires_grad=True)
    bt = torch.tensor(beta, requires_grad=True)
    m = zt.mean(0)
    v = ((zt - m) ** 2).mean(0)
    out = torch.relu((zt - m) / torch.sqrt(v + S.BN_EPS) + bt)
    out.backward(torch.tensor(dy))
    assert np.abs(ref.dz - zt.grad.numpy()).max() <= 1e-12 * scale
    assert np.abs(ref.dbeta - bt.grad.numpy()).max() <= 1e-12 * np.abs(dbeta).max()


def _fp32_emulation(b, coef):
    """Plain fp32: a sequential sum down the rows, the element formula with every operation rounded."""
    z, dy, mu, r, s = b.z, b.dy, b.mean, b.rstd, b.shift
    g = np.where(z * r + s > 0, dy, F32(0))
    xh = (z - mu) * r
    s1 = np.cumsum(g, axis=0, dtype=F32)[-1]
    s2 = np.cumsum(g * xh, axis=0, dtype=F32)[-1]
    a1, a2 = coef[0].astype(F32), coef[1].astype(F32)
    dz = r * ((g - a1) - xh * a2)
    assert s1.dtype == F32 and dz.dtype == F32
    return s1, s2, dz


@pytest.mark.parametrize("shape", B.DENSE, ids=B.shape_id)
def test_plain_fp32_stays_inside_the_bounds(shape):
    M, C = shape[:2]
    for z_bf16 in (False, True):
        b = B.build("real", M, C, z_bf16=z_bf16)
        ref = B.reference(b.z, b.dy, b.mean, b.rstd, b.shift, b.coef)
        s1, s2, dz = _fp32_emulation(b, b.coef)
        n = B.dense_chain(M)
        assert (np.abs(s1 - ref.S1) <= B.sums_tol(n, ref.A1)).all()
        assert (np.abs(s2 - ref.S2) <= B.sums_tol(n, ref.A2)).all()
        assert (np.abs(dz - ref.dz) <= B.elem_tol(ref)).all()
        assert (np.abs(B.bf16_round(dz) - ref.dz) <= B.elem_tol(ref) + B.bf16_ulp(ref.dz)).all()
        # the chain: the emulation's own coefficients against the reference's
        own = B.reference(b.z, b.dy, b.mean, b.rstd, b.shift)
        coef = np.stack([(s1.astype(np.float64) / M), (s2.astype(np.float64) / M)]).astype(F32)
        _, _, dz = _fp32_emulation(b, coef)
        assert (np.abs(dz - own.dz) <= B.elem_tol(own) + B.chain_extra(own, n)).all()


@pytest.mark.parametrize("shape", B.DENSE + B.WALK, ids=B.shape_id)
def test_exact_inputs_are_exact(shape):
    M, C = shape[:2]
    b = B.build("exact", M, C)
    B.assert_exact_grid(b)
    assert np.abs(b.dy).max() <= B.dy_range(M)
    assert np.array_equal(b.z, B.bf16_round(b.z))
    ref = B.reference(b.z, b.dy, b.mean, b.rstd, b.shift, b.coef)
    s1, s2, dz = _fp32_emulation(b, b.coef)
    assert np.array_equal(s1, ref.S1.astype(F32)) and np.array_equal(s2, ref.S2.astype(F32))
    assert np.array_equal(ref.S1.astype(F32).astype(np.float64), ref.S1)
    assert np.array_equal(dz, ref.dz.astype(F32)) and np.array_equal(ref.dz.astype(F32).astype(np.float64), ref.dz)
    if M * C >= 48:
        assert ref.mask.any() and not ref.mask.all()


@pytest.mark.parametrize("shape", B.KNIFE, ids=B.shape_id)
def test_knife_edge_inputs_split_the_fused_from_the_unfused_predicate(shape):
    M, C = shape[:2]
    b = B.build("knife", M, C)
    k = b.knife
    assert (k.sum(0) * 5 >= M).all()                                          # at least a fifth of every channel
    assert ((b.knife_sign > 0).any(0) & (b.knife_sign < 0).any(0)).all()      # both residual signs in every channel
    unfused = b.z * b.rstd + b.shift                                          # fp32, two roundings
    assert unfused.dtype == F32
    assert (unfused[k] == 0).all() and not (unfused[k] > 0).any()
    fused = b.z.astype(np.float64) * b.rstd.astype(np.float64) + b.shift      # exact: what one rounding keeps the sign of
    assert ((fused > 0) == (b.knife_sign > 0))[k].all()
    assert (fused[k] != 0).all() and (fused.astype(F32)[k] != 0).all()
    ref = B.reference(b.z, b.dy, b.mean, b.rstd, b.shift)
    assert np.array_equal(ref.mask[k], b.knife_sign[k] > 0)
    assert np.array_equal(b.dy, np.round(b.dy)) and (b.dy >= 1).all()
    # (the two masks differ on every positive knife element: the sums differ by an integer >= their count)
    assert (np.where((fused > 0) & k, b.dy, 0).sum(0) >= (b.knife_sign > 0).sum(0)).all()


@pytest.mark.parametrize("shape", B.POOLED, ids=lambda s: "%dx%dx%dx%d" % s)
def test_pooled_inputs_have_unique_window_maxima(shape):
    N, H, W, C = shape
    for mode in ("exact", "real"):
        p = B.build_pooled(mode, N, H, W, C)
        assert B.window_maxima_are_unique(p.z4)
        assert p.dy.shape == (N * H * W, C) and (p.dy_mag >= np.abs(p.dy)).all()
        assert np.abs(p.dy).sum() > 0 or N * H * W == 1
    tied = np.zeros((1, 5, 5, 4))
    assert not B.window_maxima_are_unique(tied)
    ref = B.reference(p.z, p.dy, p.mean, p.rstd, p.shift, p.coef, g_mag=p.dy_mag)
    plain = B.reference(p.z, p.dy, p.mean, p.rstd, p.shift, p.coef)
    assert (ref.mag >= plain.mag).all() and np.array_equal(ref.dz, plain.dz)
