"""ds_bn_pool_bwd_apply_cols: the BatchNorm + ReLU backward apply of a column range of a layer behind a stride-2 SAME max pool
(3x3/2: MaxPool_4a behind Mixed_3c, 2x2/2: MaxPool_5a behind Mixed_4f), straight from the POOLED gradient and the winners.
(a) dz has the bits of ds_maxpool_bwd followed by ds_bn_bwd_apply on the same inputs; (b) dz agrees with the fp64 oracle's
MaxPoolGrad + BatchNorm backward within the bound the ds_bn_pool_bwd_apply / ds_bn_bwd_apply kernel tests use (2e-4 of the
largest reference value).  z is quantised to multiples of 1/4, so most windows tie, many activations are negative and -- in the
channels whose rstd is a power of two -- exactly zero.  ds_bn_bwd_apply_cols (the dense parts of the same layer) is held to
ds_bn_bwd_apply's bits on the column range."""
import functools

import numpy as np
import pytest
import torch

from oracle import tf_semantics as S

pytestmark = pytest.mark.gpu

N, CP, C0 = 2, 20, 8           # pool width 20, the column range [8, 20)
NC = CP - C0
SHAPES = [(3, 9, 9), (3, 8, 8), (3, 7, 5), (2, 6, 6), (2, 7, 7)]      # (k, H, W): padding on both sides / bottom-right only / none


def dev(a, dtype=torch.float32):
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda")


@functools.lru_cache(maxsize=None)
def _case(k, H, W):
    """Inputs, the two-launch result on the device and the fp64 oracle of one shape: computed once, shared, never written."""
    from tumblr_emotions_amd import ops
    rng = np.random.RandomState(100 * k + 10 * H + W)
    z = np.round(rng.normal(0.1, 0.8, size=(N, H, W, CP)) * 4) / 4
    mean = np.round(rng.normal(0.1, 0.3, size=CP) * 4) / 4
    rstd = rng.uniform(0.5, 2.0, size=CP).astype(np.float32)
    rstd[::3] = np.array([0.5, 2.0, 1.0, 0.5, 2.0, 1.0, 0.5])[:len(rstd[::3])]      # beta = 0 there: z == mean gives exactly 0
    beta = (rng.normal(size=CP) * 0.3).astype(np.float32)
    beta[::3] = 0.0
    shift = (beta - (mean.astype(np.float32) * rstd)).astype(np.float32)
    coef = (rng.normal(size=(2, CP)) * 0.1).astype(np.float32)
    OH, OW = -(-H // 2), -(-W // 2)
    dpool = rng.normal(size=(N, OH, OW, CP)).astype(np.float32)
    zd, md, rd, sd, cd, dpd = dev(z), dev(mean), dev(rstd), dev(shift), dev(coef), dev(dpool)
    yp = torch.empty(N, OH, OW, CP, device="cuda")
    am = torch.empty(N, OH, OW, CP, dtype=torch.uint8, device="cuda")
    ops.maxpool_bn_relu_fwd(zd, rd, sd, yp, am, N, H, W, CP, k, 2)          # the winners the backward kernels consume
    # the two launches this kernel replaces
    full = torch.full((N, H, W, CP), float("nan"), device="cuda")
    ops.maxpool_bwd(dpd, am, full, False, N, H, W, CP, k, 2, "SAME")
    M = N * H * W
    z2 = zd.view(M, CP)
    wide = torch.zeros(M, CP, device="cuda")          # (ds_bn_bwd_apply writes dz with z's row stride)
    segs = ops.make_segments([(0, NC, full.data_ptr() + 4 * C0, CP)])
    ops.bn_bwd_apply(z2[:, C0:], segs, M, NC, md[C0:], rd[C0:], sd[C0:], cd[:, C0:].contiguous(), wide[:, C0:], ldz=CP)
    torch.cuda.synchronize()
    two = wide[:, C0:].contiguous()
    # fp64 oracle on the same fp32 vectors
    r64, s64, m64 = rstd.astype(np.float64), shift.astype(np.float64), mean.astype(np.float64)
    pre = z * r64 + s64
    y = np.maximum(pre, 0.0)
    dy_full = S.max_pool_bwd(y, dpool.astype(np.float64), k, 2, "SAME")
    g = dy_full * (pre > 0)
    xhat = (z - m64) * r64
    ref = r64 * (g - coef[0].astype(np.float64) - xhat * coef[1].astype(np.float64))
    zeros = float((pre[..., C0:] == 0).mean()), float((pre[..., C0:] <= 0).mean())
    return dict(z=zd, mean=md, rstd=rd, shift=sd, coef=cd, dpool=dpd, am=am, two=two, ref=ref[..., C0:].reshape(M, NC), M=M,
                zeros=zeros)


def _check(dz, c):
    assert torch.equal(dz, c["two"]), "differs from ds_maxpool_bwd + ds_bn_bwd_apply in %d elements" % int((dz != c["two"]).sum())
    err = np.abs(dz.cpu().numpy().astype(np.float64) - c["ref"]).max()
    scale = max(1e-6, np.abs(c["ref"]).max())
    print("max err %.3e of scale %.3e" % (err, scale))
    assert err <= 2e-4 * scale, "max err %.3e vs scale %.3e" % (err, scale)


@pytest.mark.parametrize("k,H,W", SHAPES)
def test_own_buffer_has_the_bits_of_the_two_launches_and_matches_the_oracle(k, H, W):
    """z of the range in its own 12-wide buffer, dz into a separate 16-wide one (columns 12.. untouched)."""
    from tumblr_emotions_amd import ops
    c = _case(k, H, W)
    M = c["M"]
    assert c["zeros"][0] > 0.002 and c["zeros"][1] > 0.3, c["zeros"]            # the inputs do sit at and below zero
    z12 = c["z"].view(M, CP)[:, C0:].contiguous()
    keep = z12.clone()
    dz = torch.full((M, 16), 7.0, device="cuda")
    ops.bn_pool_bwd_apply_cols(z12, NC, dz, 16, c["dpool"], c["am"], CP, C0, N, H, W, NC, c["mean"][C0:], c["rstd"][C0:],
                               c["shift"][C0:], c["coef"][0, C0:], c["coef"][1, C0:], k)
    torch.cuda.synchronize()
    _check(dz[:, :NC].contiguous(), c)
    assert torch.equal(z12, keep) and float((dz[:, NC:] - 7.0).abs().max()) == 0.0


@pytest.mark.parametrize("k,H,W", SHAPES)
def test_in_place_inside_the_wider_buffer(k, H, W):
    """z as columns 8.. of a 20-wide buffer, differentiated in place; columns [0, 8) stay as they are."""
    from tumblr_emotions_amd import ops
    c = _case(k, H, W)
    M = c["M"]
    wide = c["z"].clone().view(M, CP)
    view = wide[:, C0:]
    ops.bn_pool_bwd_apply_cols(view, CP, view, CP, c["dpool"], c["am"], CP, C0, N, H, W, NC, c["mean"][C0:], c["rstd"][C0:],
                               c["shift"][C0:], c["coef"][0, C0:], c["coef"][1, C0:], k)
    torch.cuda.synchronize()
    _check(wide[:, C0:].contiguous(), c)
    assert torch.equal(wide[:, :C0], c["z"].view(M, CP)[:, :C0])


def test_dense_column_range_has_the_bits_of_the_whole_layer_pass():
    """ds_bn_bwd_apply_cols on the columns [8, 24) of a 24-column layer (two gradient segments with strides of their own, in
    place with ldz = 24) against ds_bn_bwd_apply over the whole layer."""
    from tumblr_emotions_amd import ops
    rng = np.random.RandomState(3)
    M, Cc, c0 = 331, 24, 8
    z = dev(np.round(rng.normal(size=(M, Cc)) * 4) / 4)
    d0, d1, d2 = dev(rng.normal(size=(M, 8))), dev(rng.normal(size=(M, 12))), dev(rng.normal(size=(M, 8)))
    mean, shift = dev(rng.normal(size=Cc) * 0.2), dev(rng.normal(size=Cc) * 0.2)
    rstd = dev(rng.uniform(0.5, 2.0, size=Cc))
    coef = dev(rng.normal(size=(2, Cc)) * 0.1)
    whole = z.clone()
    ops.bn_bwd_apply(whole, ops.make_segments([(0, 8, d0.data_ptr(), 8), (8, 20, d1.data_ptr(), 12), (20, 24, d2.data_ptr(), 8)]),
                     M, Cc, mean, rstd, shift, coef, whole)
    part = z.clone()
    view = part[:, c0:]
    ops.bn_bwd_apply_cols(view, ops.make_segments([(0, 12, d1.data_ptr(), 12), (12, 16, d2.data_ptr(), 8)]), M, Cc - c0,
                          mean[c0:], rstd[c0:], shift[c0:], coef[0, c0:], coef[1, c0:], view, ldz=Cc)
    torch.cuda.synchronize()
    assert torch.equal(part[:, c0:], whole[:, c0:]) and torch.equal(part[:, :c0], z[:, :c0])
