"""Branch_3's MaxPool 3x3 / 1 formed on load by the wide 1x1 kernel (ds_conv_desc.pool_argmax), shape by shape: the loader
fetches a workgroup's centre rows once into an LDS tile and takes the rows above and below from there, so the cases sit where
that can go wrong -- a workgroup whose four blocks straddle two images, surplus waves behind the last image, halo rows that
come from memory (first block of a workgroup) next to halo rows that come from the tile, one K step and many, a ragged column
tile, maps of one pixel and of a width that does not divide 32."""
import functools

import numpy as np
import pytest
import torch

from oracle import tf_semantics as S

pytestmark = pytest.mark.gpu


def _ops():
    from tumblr_emotions_amd import ops
    return ops


def dev(a, dtype=torch.float32):
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda")


def close(got, ref, tol=2e-4):
    got = got.detach().cpu().numpy().astype(np.float64)
    scale = max(1e-6, np.abs(ref).max())
    err = np.abs(got - ref).max()
    assert err <= tol * scale, "max err %.3e vs scale %.3e" % (err, scale)


# (N, H, W): 28 x 28 -- one image row per block, 28 blocks per image; 14 x 14 with N = 3 -- seven blocks per image, 21 blocks:
# workgroups 1, 3 and 5 straddle two images and the last one has three surplus waves; 7 x 7 with N = 5 -- two blocks per image
# (four rows and three), every workgroup holds two images and the last one has two surplus waves
MAPS = [(2, 28, 28), (3, 14, 14), (5, 7, 7)]
CASES = ([m + (K, 32, norm) for m in MAPS for K in (16, 48, 832) for norm in (False, True)] +
         [m + (48, 40, norm) for m in MAPS for norm in (False, True)] +                     # a ragged column tile
         [(1, 1, 1, 32, 32, True), (1, 1, 1, 32, 32, False), (3, 9, 11, 48, 96, True), (3, 9, 11, 48, 96, False),
          (2, 5, 32, 64, 40, False)])


@functools.lru_cache(maxsize=None)
def _problem(case):
    """Inputs on a coarse grid (exact ties inside most windows; post-ReLU, or raw z with a Branch_0 slice of activations when
    `norm`), and the fp64 oracle: the pooled activation, its winners and the conv output."""
    N, H, W, K, Nc, norm = case
    rng = np.random.RandomState(11 + H + K + Nc)
    x = np.round(rng.normal(size=(N, H, W, K)) * 3) / 3
    r = (np.abs(rng.normal(size=K)) + 0.5).astype(np.float32)
    sh = (rng.normal(size=K) * 0.3).astype(np.float32)
    if norm:
        r[:K // 4], sh[:K // 4] = 1.0, 0.0
        x[..., :K // 4] = np.maximum(x[..., :K // 4], 0)
    else:
        x = np.maximum(x, 0)
    w = (rng.normal(size=(K, Nc)) * 0.1).astype(np.float32)
    pivot = (rng.normal(size=Nc) * 0.1).astype(np.float32)
    y = np.maximum(x * r + sh, 0) if norm else x
    # (the winners are taken over the raw values: rstd > 0, so they are the winners of y wherever y's maximum is positive,
    # and the two-launch form below is the byte-for-byte reference everywhere)
    ref = S.max_pool(y, 3, 1, "SAME").reshape(N * H * W, K) @ w.astype(np.float64)
    for a in (x, r, sh, w, pivot, ref):
        a.setflags(write=False)
    return x, r, sh, w, pivot, ref, S.max_pool_argmax(x, 3, 1, "SAME")


@pytest.mark.parametrize("case", CASES)
def test_pool_on_load_equals_pool_then_plain_wide_launch(case, tuning_lib):
    """One launch with ds_conv_desc.pool_argmax against ds_maxpool_fwd / ds_maxpool_bn_relu_fwd followed by the plain launch
    of the wide kernel: z equal to the bit (the same MFMA sequence per output element; at K = 16, where the plain form is
    not a wide-kernel launch, within the rounding of two fp32 sums of 16 products), the winners equal byte for byte and
    every byte of them written (the buffer is pre-filled with 77), the guard rows behind z untouched, the statistics equal up
    to the grouping of the partial sums (1e-5), and everything within 2e-4 of the fp64 oracle."""
    ops = _ops()
    lib = tuning_lib          # (the same kernel sources + ds_debug_conv_set_wide)
    N, H, W, K, Nc, norm = case
    x, r, sh, w, pivot, ref, am_oracle = _problem(case)
    xt, rt, st, wt, pv = dev(x), dev(r), dev(sh), dev(w), dev(pivot)
    M = N * H * W
    pooled = torch.empty(N, H, W, K, device="cuda")
    am_ref = torch.empty(N, H, W, K, dtype=torch.uint8, device="cuda")
    if norm:
        ops.maxpool_bn_relu_fwd(xt, rt, st, pooled, am_ref, N, H, W, K, 3, 1)
    else:
        ops.maxpool_fwd(xt, pooled, am_ref, N, H, W, K, 3, 1, "SAME")
    beta = torch.zeros(Nc, device="cuda")

    def run(fused):
        plan = ops.LayerPlan(ops.DS_CONV_FWD, ops.DS_ARITH_F32, 0, N, H, W, K, Nc, 1, 1, K, Nc, ops.DS_EPI_STATS)
        am = torch.full((N, H, W, K), 77, dtype=torch.uint8, device="cuda")
        if fused:
            assert plan.enable_pool3(am)
            if norm:
                plan.d.norm_rstd, plan.d.norm_shift = rt.data_ptr(), st.data_ptr()
        z = torch.full((M + 3, Nc), 5.0, device="cuda")
        stats = torch.zeros(2 * Nc * plan.partials, device="cuda")
        plan.run(ops._p(xt if fused else pooled), ops._p(wt), ops._p(z), stats=ops._p(stats), pivot=ops._p(pv))
        mean, rstd, shift = (torch.empty(Nc, device="cuda") for _ in range(3))
        ops.bn_finalize(stats, plan.partials, M, Nc, beta, 1e-3, 0.9997, mean, rstd, shift, None, None, pivot=pv)
        torch.cuda.synchronize()
        assert float((z[M:] - 5.0).abs().max()) == 0.0
        return z[:M], am, mean, rstd

    lib.ds_debug_conv_set_wide(2)          # the plain launch on the wide kernel wherever the shape allows it
    try:
        z0, _, mean0, rstd0 = run(False)
    finally:
        lib.ds_debug_conv_set_wide(1)
    z1, am1, mean1, rstd1 = run(True)
    assert torch.equal(am1, am_ref), "winners differ at %d of %d positions" % (int((am1 != am_ref).sum()), am_ref.numel())
    if not norm:
        assert np.array_equal(am1.cpu().numpy(), am_oracle)
    nbad = int((z0 != z1).sum())
    print("case %s: z differs from the two-launch form at %d of %d elements, max %.3e" %
          (case, nbad, z0.numel(), float((z0 - z1).abs().max())))
    if K >= 32:
        assert torch.equal(z0, z1)
    else:
        # one K step: the plain form stays on the LDS-tile kernels (the wide kernel takes Cin >= 32), which add the 16
        # products in another order.  Each fp32 sum is within K * 2^-24 * sum |a b| of the exact one, the two within twice that.
        bound = (pooled.reshape(M, K).abs() @ wt.abs()) * (K * 2.0 ** -23)
        assert bool(((z0 - z1).abs() <= bound).all())
    close(z1, ref)
    close(z0, ref)
    assert float((mean0 - mean1).abs().max()) <= 1e-5 * max(1.0, float(mean0.abs().max()))
    if M >= 64:          # (a single pixel has variance 0: rstd = eps^-1/2 amplifies the last bit of the two groupings)
        assert float((rstd0 - rstd1).abs().max()) <= 1e-5 * float(rstd0.abs().max())
    close(mean1, ref.mean(0), 1e-4)


def test_pool_on_load_is_one_column_tile():
    """The pooling is the loader's work and would be redone per column tile, so the plan forms it on load for one column tile
    only (Cout <= 128; the recorded plan table holds that answer): at Cout = 160 the layer keeps the two-launch form, which
    is why the kernel has no winner stores to suppress in a second column tile."""
    ops = _ops()
    am = torch.full((2, 14, 14, 48), 77, dtype=torch.uint8, device="cuda")
    plan = ops.LayerPlan(ops.DS_CONV_FWD, ops.DS_ARITH_F32, 0, 2, 14, 14, 48, 160, 1, 1, 48, 160, ops.DS_EPI_STATS)
    assert not plan.enable_pool3(am)
    assert not plan.d.pool_argmax
    plan = ops.LayerPlan(ops.DS_CONV_FWD, ops.DS_ARITH_F32, 0, 2, 14, 14, 48, 128, 1, 1, 48, 128, ops.DS_EPI_STATS)
    assert plan.enable_pool3(am)
