"""gemm_wide_kernel (the wide 1x1 kernel) against the fp64 reference, instantiation by instantiation: the case table of
wide_cases.py under ds_debug_conv_set_wide_nb, every launch checked with ds_debug_conv_igemm_launch to be the intended
instantiation before it runs.  Exact operands: z, the statistics partials and the winners' bytes EQUAL the reference, z sits
between guards, the statistics start as NaN with a canary behind, the inputs are unchanged afterwards.  One real-valued launch
per instantiation, with the bit-identity twins the project promises (BatchNorm + ReLU on load against ds_bn_apply_relu + the
plain launch, BatchNorm backward on load against ds_bn_bwd_apply + the plain dgrad, at the same pinned NB)."""
import ctypes as C

import numpy as np
import pytest
import torch

import wide_cases as W

pytestmark = pytest.mark.gpu

REACHED, REAL_REACHED = set(), set()
WORST = {}


def _ops():
    from tumblr_emotions_amd import ops
    return ops


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class Launch:
    """One launch of a problem: the device operands (kept for the unchanged-inputs check), the outputs copied back."""

    def __init__(self, lib, p, x=None, on_load=True):
        from tumblr_emotions_amd import _lib
        ops = _ops()
        c = p.case
        self.p = p
        self.inputs = []          # (device tensor, host array it was made from)

        def put(a):
            t = dev(a)
            self.inputs.append((t, a))
            return t

        xt = put(p.x) if x is None else x
        wt = put(p.w)
        zbuf = dev(W.z_buffer(p))
        z_ptr = C.c_void_p(zbuf.data_ptr() + W.GUARD_ROWS * c.ldz * 4)
        sums = c.flags & (W.EPI_STATS | W.EPI_BNSUMS)
        stats = dev(W.stats_buffer(p)) if sums else None
        mask = put(p.mask) if p.mask is not None else None
        pivot = put(p.pivot) if p.pivot is not None else None
        am = dev(W.winners_buffer(p)) if c.pool else None
        norm = c.norm and on_load
        bnb = c.bnb and on_load
        inst = (c.nb, int(c.n_contig), int(bnb), int(c.pool), int(c.bnr))
        keep = []
        if norm:
            keep += [put(p.rstd), put(p.shift)]
        if bnb:
            b = p.bnb
            bl = _lib.BnBwdOnLoad()
            self.bn = [put(b.mean), put(b.rstd), put(b.shift), put(b.coef)]
            bl.mean, bl.rstd, bl.shift, bl.coef = (t.data_ptr() for t in self.bn)
            bl.nseg = len(p.dy_parts)
            self.parts = []
            for i, (c0, c1, part) in enumerate(p.dy_parts):
                t = put(part)
                bl.c_end[i], bl.ld[i], bl.dy[i] = c1, part.shape[1], t.data_ptr()
                self.parts.append((c0, c1, t.data_ptr(), part.shape[1]))
            keep.append(bl)
        with W.pinned(lib, c.nb):
            if c.bnr:
                n, h, w = c.hw if c.pool else (c.M, 1, 1)
                plan = ops.LayerPlan(ops.DS_CONV_FWD, ops.DS_ARITH_F32, 0, n, h, w, c.K, c.Cout, 1, 1, c.ldx, c.ldz, 0)
                assert plan.family == ops.DS_FAM_IGEMM
                if c.pool:
                    assert plan.enable_pool3(am)
                if norm:
                    plan.d.norm_rstd, plan.d.norm_shift = keep[0].data_ptr(), keep[1].data_ptr()
                plan = plan.bn_relu_variant()
                assert plan is not None
                d = plan.d
                scale, shift = put(p.scale), put(p.bn_shift)
            else:
                d = W.make_desc(c)
                if norm:
                    d.norm_rstd, d.norm_shift = keep[0].data_ptr(), keep[1].data_ptr()
                if bnb:
                    d.bnb = C.addressof(keep[-1])
                if c.pool:
                    d.pool_argmax = am.data_ptr()
                if p.mask_rstd is not None:
                    keep += [put(p.mask_rstd), put(p.mask_shift)]
                    d.mask_rstd, d.mask_shift = keep[-2].data_ptr(), keep[-1].data_ptr()
            # the intended instantiation is the one chosen, on the grid and with the partial count the table states
            got = W.launch_of(lib, d)
            _, wgs, partials = W.expected_launch(c)
            assert got[:5] == inst and got[8] == wgs and got[9] == partials, (c, got)
            if c.bnr:
                plan.run_bn_relu(ops._p(xt), ops._p(wt), z_ptr, scale.data_ptr(), shift.data_ptr())
            else:
                if sums:
                    d.partials = partials
                _lib.check(lib.ds_conv_igemm(C.byref(d), ops._p(xt), ops._p(wt), z_ptr, None, ops._p(mask), ops._p(stats),
                                             ops._p(pivot), ops._stream()), "ds_conv_igemm")
            torch.cuda.synchronize()
        self.inst = inst
        self.zbuf = zbuf.cpu().numpy()
        self.z = self.zbuf[W.GUARD_ROWS:W.GUARD_ROWS + c.M, :c.Cout]
        self.stats = stats.cpu().numpy() if sums else None
        self.winners = am.cpu().numpy() if c.pool else None
        for t, a in self.inputs:          # z under the BatchNorm backward on load in particular
            assert np.array_equal(t.cpu().numpy(), a, equal_nan=True), "%r: an input changed" % (c,)


@pytest.mark.parametrize("variant,nb", W.VARIANT_NB)
def test_exact_operands_equal_the_fp64_reference(variant, nb, tuning_lib):
    """Integer / dyadic operands (wide_cases.build asserts that every fp32 order is exact): z, every statistics partial (per
    column total under POOL, whose partials group other rows) and every winner byte equal the fp64 reference; guard rows,
    guard columns and the canaries intact; every partial and every winner byte written; inputs unchanged."""
    lib = tuning_lib
    try:
        for c in W.cases(variant, nb):
            p = W.build(c)
            r = Launch(lib, p)
            W.check_z(r.zbuf, p)
            if r.stats is not None:
                W.check_stats(r.stats, p)
            if c.pool:
                W.check_winners(r.winners, p)
            REACHED.add(r.inst)
        print("wide exact %s nb %d: %d launches of gemm_wide_kernel<%d, %d, %d, %d, %d>" % ((variant, nb, len(W.cases(variant, nb))) + r.inst))
    finally:
        lib.ds_debug_conv_set_wide(1)
        lib.ds_debug_conv_set_wide_nb(0)


def _outside_is_guard(r):
    c = r.p.case
    out = r.zbuf.copy()
    out[W.GUARD_ROWS:W.GUARD_ROWS + c.M, :c.Cout] = W.GUARD
    assert np.array_equal(out, np.full_like(out, W.GUARD)), "%r: a guard of z was overwritten" % (c,)


@pytest.mark.parametrize("variant,nb", W.VARIANT_NB)
def test_real_operands_stay_inside_the_bounds_and_the_twins_agree_to_the_bit(variant, nb, tuning_lib):
    """Normal operands, so that exactness cannot hide a precision loss: z within 2e-4 max|ref| (test_kernels_gpu.py's gate),
    the sums within (128 + 4) 2^-24 sum|term| per partial of fp64 sums over the kernel's OWN stored z, the winners equal.  The
    on-load variants against their two-launch forms at the same pin: equal bits."""
    ops = _ops()
    lib = tuning_lib
    try:
        c = W.real_case(variant, nb)
        p = W.build(c)
        r = Launch(lib, p)
        _outside_is_guard(r)
        scale = max(1e-6, np.abs(p.z).max())
        zerr = np.abs(r.z.astype(np.float64) - p.z).max() / (W.Z_TOL * scale)
        print("wide real %s nb %d %r: z error %.3f of its bound" % (variant, nb, c, zerr))
        assert zerr <= 1.0
        serr = None
        if r.stats is not None:
            serr = W.real_stats_check(r.stats, p, r.z)
            print("wide real %s nb %d: sums error %.3f of their bound" % (variant, nb, serr))
        if c.pool:
            W.check_winners(r.winners, p)
        key = "gemm_wide_kernel<%d, %d, %d, %d, %d>" % r.inst
        WORST[key] = (max(WORST.get(key, (0, 0))[0], zerr), max(WORST.get(key, (0, 0))[1], serr or 0.0))
        REAL_REACHED.add(r.inst)
        if variant == "norm":
            y = torch.full((c.M, c.ldx), W.X_PAD, device="cuda")
            zt, rt, st = dev(p.x[:, :c.K]), dev(p.rstd), dev(p.shift)
            ops.bn_apply_relu(zt, c.M, c.K, rt, st, ops.make_segments([(0, c.K, y.data_ptr(), c.ldx)]))
            t = Launch(lib, p, x=y, on_load=False)
            assert np.array_equal(t.zbuf, r.zbuf) and np.array_equal(t.stats, r.stats)
        if variant == "bnb":
            b = p.bnb
            dz = dev(p.x)
            md, rd, sd, cd = dev(b.mean), dev(b.rstd), dev(b.shift), dev(b.coef)
            parts = [(c0, c1, dev(part)) for c0, c1, part in p.dy_parts]
            segs = ops.make_segments([(c0, c1, t_.data_ptr(), t_.shape[1]) for c0, c1, t_ in parts])
            ops.bn_bwd_apply(dz, segs, c.M, c.K, md, rd, sd, cd, dz, ldz=c.ldx)
            torch.cuda.synchronize()
            assert float((dz[:, c.K:] - W.X_PAD).abs().max()) == 0.0
            t = Launch(lib, p, x=dz, on_load=False)
            assert t.inst == (c.nb, 0, 0, 0, 0)
            assert np.array_equal(t.zbuf, r.zbuf) and np.array_equal(t.stats, r.stats)
    finally:
        lib.ds_debug_conv_set_wide(1)
        lib.ds_debug_conv_set_wide_nb(0)


def test_the_cases_reach_every_instantiation():
    """Run after the cases above (same module): the exact table and the real-valued launches each ran all 34 instantiations of
    gemm_wide_kernel that kernel_of() names -- a launch that lands on another one fails its own assertion, an instantiation
    nobody reaches fails here."""
    if not REACHED and not REAL_REACHED:
        pytest.skip("needs the cases of this module in the same session")      # (only when selected alone)
    assert len(W.ALL_INSTANTIATIONS) == 34
    assert REACHED == W.ALL_INSTANTIATIONS, sorted(W.ALL_INSTANTIATIONS - REACHED)
    assert REAL_REACHED == W.ALL_INSTANTIATIONS, sorted(W.ALL_INSTANTIATIONS - REAL_REACHED)
    for k in sorted(WORST):
        print("test_wide_gpu: %s real-valued z %.3f, sums %.3f of their bounds" % ((k,) + WORST[k]))
