"""The batch-statistics BatchNorm + ReLU backward against fp64, every entry point at its edges: ds_bn_bwd_reduce, the three
finalize kernels, the ds_bn_bwd_apply family (in place, bf16 out, bf16 z, a column range, the max|dz| record) and the pooled
twins ds_bn_pool_bwd_reduce / _apply.  Reference, bounds and inputs: tests/bn_bwd_ref.py (checked on their own by
tests/test_bn_bwd_ref_cpu.py).  Every tolerance is computed there from the inputs; every element takes part in every
comparison.  A line `ANCHOR ...` reports the largest error of a comparison as a fraction of its bound before the assertion."""
import ctypes

import numpy as np
import pytest
import torch

import bn_bwd_ref as B

pytestmark = pytest.mark.gpu

SENT = -777.25            # on no grid of the exact inputs
SENT16 = -776.0           # the same for a bf16 tensor (exactly representable there)
GUARD = 64
F32 = np.float32


def _ops():
    from tumblr_emotions_amd import ops
    return ops


def _cuda(a, dtype=torch.float32):
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


def _guarded(n, fill=SENT, dtype=torch.float32):
    """A tensor of n elements between two guards of sentinels: (whole buffer, view of the n elements)."""
    buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device="cuda")
    return buf, buf[GUARD:GUARD + n]


def _guards_intact(buf, fill=SENT):
    return bool((buf[:GUARD] == fill).all()) and bool((buf[-GUARD:] == fill).all())


def _bits(t):
    t = t.contiguous()
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _np(t):
    return t.float().cpu().numpy()


def _within(what, err, bound):
    """Report the largest error as a fraction of its bound, then assert err <= bound at every element."""
    err, bound = np.asarray(err, np.float64), np.broadcast_to(np.asarray(bound, np.float64), np.shape(err))
    safe = np.where(bound > 0, bound, 1.0)
    ratio = np.where(bound > 0, err / safe, np.where(err > 0, np.inf, 0.0))
    print("ANCHOR %s: largest error / bound = %.3f (largest error %.3e)" % (what, float(ratio.max()), float(err.max())))
    assert (err <= bound).all(), what


def _bit_equal(what, got, want32):
    """got (fp32 values on the host) has the bits of the reference cast to fp32."""
    bad = int((np.ascontiguousarray(got, F32).view(np.uint32) != np.ascontiguousarray(want32, F32).view(np.uint32)).sum())
    print("ANCHOR %s: %d of %d elements differ from the reference's bits" % (what, bad, np.size(got)))
    assert bad == 0, what


class Dev:
    """The device side of a dense case: z [M, ldz] with NaN in the columns >= C, every dy segment in a buffer of its own whose
    row stride is wider than the segment (sentinels in the slack), the per-channel vectors."""

    def __init__(self, b, shape, z16=False):
        ops = _ops()
        M, C, ldz, cuts = shape
        zh = np.full((M, ldz), np.nan, F32)
        zh[:, :C] = b.z
        self.z = _cuda(zh)
        self.z16 = self.z.to(torch.bfloat16) if z16 else None
        if z16:
            assert _same_bits(self.z16[:, :C].float(), self.z[:, :C])          # z is bf16-exact
        self.keep, self.want, parts = [], [], []
        for i, (c0, c1) in enumerate(zip(cuts[:-1], cuts[1:])):
            ld = (c1 - c0) + 4 * (i + 1)
            buf = np.full((M, ld), SENT, F32)
            buf[:, :c1 - c0] = b.dy[:, c0:c1]
            t = _cuda(buf)
            self.keep.append(t)
            self.want.append(t.clone())
            parts.append((c0, c1, t.data_ptr(), ld))
        self.parts = parts
        self.segs = ops.make_segments(parts)
        self.mean, self.rstd, self.shift = _cuda(b.mean), _cuda(b.rstd), _cuda(b.shift)
        self.coef = _cuda(b.coef)
        self.z0, self.z16_0 = self.z.clone(), (self.z16.clone() if z16 else None)
        self.shape = shape

    def assert_inputs_intact(self, z_too=True):
        """After every call: z (its NaN columns included), the gradient segments and the sentinels in their slack."""
        if z_too:
            assert _same_bits(self.z, self.z0)
            if self.z16 is not None:
                assert _same_bits(self.z16, self.z16_0)
        for t, w in zip(self.keep, self.want):
            assert torch.equal(t, w)


def _partial_sums(part, C, P):
    return part[:2 * C * P].cpu().numpy().astype(np.float64).reshape(2, C, P).sum(2)


# ---- 1. reduce --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", B.DENSE, ids=B.shape_id)
@pytest.mark.parametrize("mode", ["exact", "real"])
def test_reduce_sums_every_element_once(mode, shape):
    """ds_bn_bwd_reduce, fp32 z and bf16 z (ldz > C included): exact inputs give the reference's integers whatever the thread
    layout (C / 4 not dividing 256, more row groups than rows, one row group, the 4-row trip and its tail, a short last block,
    M = 1, segment cuts at odd multiples of 4); real inputs stay inside (n + 4) u sum|term|.  A second launch has the same
    bits."""
    ops = _ops()
    M, C, ldz, cuts = shape
    P = ops.bn_bwd_partials(M, C)
    assert 1 <= P <= M
    n = B.dense_chain(M)
    for z16 in (False, True):
        b = B.build(mode, M, C, z_bf16=z16)
        ref = B.reference(b.z, b.dy, b.mean, b.rstd, b.shift)
        d = Dev(b, shape, z16)
        parts = []
        for _ in range(2):
            buf, part = _guarded(2 * C * P)
            ops.bn_bwd_reduce(d.z16 if z16 else d.z, d.segs, M, C, d.mean, d.rstd, d.shift, part, ldz=ldz)
            torch.cuda.synchronize()
            d.assert_inputs_intact()
            assert _guards_intact(buf) and bool((part != SENT).all())          # P partials per channel, no more, no fewer
            parts.append(part)
        assert _same_bits(parts[0], parts[1])
        got = _partial_sums(parts[0], C, P)
        what = "reduce %s %s %s" % (mode, B.shape_id(shape), "bf16 z" if z16 else "fp32 z")
        if mode == "exact":
            _bit_equal(what + " sum g", got[0].astype(F32), ref.S1.astype(F32))
            _bit_equal(what + " sum g*xhat", got[1].astype(F32), ref.S2.astype(F32))
            assert np.array_equal(got[0], ref.S1) and np.array_equal(got[1], ref.S2)
        else:
            _within(what + " sum g", np.abs(got[0] - ref.S1), B.sums_tol(n, ref.A1))
            _within(what + " sum g*xhat", np.abs(got[1] - ref.S2), B.sums_tol(n, ref.A2))


# ---- 2. finalize ------------------------------------------------------------------------------------------------------------
def _check_finalized(what, integer, M, s, q, abs_s, abs_q, dbeta, coef):
    """dbeta (or None) and coef (or None) against the fp64 sums s, q [C] of the partials."""
    if dbeta is not None:
        if integer:
            _bit_equal(what + " dbeta", dbeta, s.astype(F32))
        else:
            _within(what + " dbeta", np.abs(dbeta - s), B.finalize_tol(s, abs_s))
    if coef is not None:
        for k, (v, a) in enumerate(((s, abs_s), (q, abs_q))):
            if integer:                                   # (M is a power of two there: 1 / M is exact)
                _bit_equal(what + " coef[%d]" % k, coef[k], (v / M).astype(F32))
            else:
                _within(what + " coef[%d]" % k, np.abs(coef[k] - v / M), B.finalize_tol(v / M, a / M))


@pytest.mark.parametrize("P", [1, 255, 256, 257, 1000])
def test_finalize_adds_every_partial_once(P):
    """ds_bn_bwd_finalize from hand-made partials [2][C][P], P on either side of the 256 threads of a workgroup, with and
    without coef.  Small integers: the bits of the fp64 sums.  Sentinels around every output stay."""
    ops = _ops()
    C = 12
    rng = np.random.RandomState(P)
    for integer in (True, False):
        M = 1024 if integer else 1000
        parts = (rng.randint(-8, 9, size=(2, C, P)) if integer else rng.normal(size=(2, C, P)) * 3).astype(F32)
        p64 = parts.astype(np.float64)
        s, q, abs_s, abs_q = p64[0].sum(1), p64[1].sum(1), np.abs(p64[0]).sum(1), np.abs(p64[1]).sum(1)
        pbuf, pd = _guarded(2 * C * P)
        pd.copy_(_cuda(parts.reshape(-1)))
        for with_coef in (True, False):
            dbuf, dbeta = _guarded(C)
            cbuf, coef = _guarded(2 * C)
            ops.bn_bwd_finalize(pd, P, M, C, dbeta, coef if with_coef else None)
            torch.cuda.synchronize()
            assert _guards_intact(dbuf) and _guards_intact(cbuf) and _guards_intact(pbuf)
            assert _same_bits(pd, _cuda(parts.reshape(-1)))
            if not with_coef:
                assert bool((coef == SENT).all())
            _check_finalized("finalize P=%d integer=%s coef=%s" % (P, integer, with_coef), integer, M, s, q, abs_s, abs_q,
                             _np(dbeta), _np(coef).reshape(2, C) if with_coef else None)


def test_finalize_segs_and_multi_route_four_producers():
    """ds_bn_bwd_finalize_segs / _multi: four segments cut at channels 4, 12, 28 (4-aligned, not 8-aligned), P = 1, 255, 257,
    1000 and kinds 0, 1, 1, 0 (kind 1: q - beta * s).  _multi with one dbeta vector missing."""
    ops = _ops()
    C, cuts, Ps, kinds = 40, (0, 4, 12, 28, 40), (1, 255, 257, 1000), (0, 1, 1, 0)
    rng = np.random.RandomState(40)
    for integer in (True, False):
        M = 1024 if integer else 1000
        beta = (rng.randint(-2, 3, size=C) if integer else rng.normal(size=C)).astype(F32)
        s, q, abs_s, abs_q = (np.zeros(C) for _ in range(4))
        sg = ops.SumSegments()
        sg.nseg = 4
        keep = []
        for i, (c0, c1) in enumerate(zip(cuts[:-1], cuts[1:])):
            n, P = c1 - c0, Ps[i]
            parts = (rng.randint(-8, 9, size=(2, n, P)) if integer else rng.normal(size=(2, n, P)) * 3).astype(F32)
            p64 = parts.astype(np.float64)
            s[c0:c1], abs_s[c0:c1] = p64[0].sum(1), np.abs(p64[0]).sum(1)
            q[c0:c1], abs_q[c0:c1] = p64[1].sum(1), np.abs(p64[1]).sum(1)
            if kinds[i] == 1:
                q[c0:c1] -= beta[c0:c1].astype(np.float64) * s[c0:c1]
                abs_q[c0:c1] += np.abs(beta[c0:c1].astype(np.float64)) * abs_s[c0:c1]
            ts, tq = _cuda(parts[0]), _cuda(parts[1])                 # the two planes in buffers of their own
            keep += [ts, tq]
            sg.c_begin[i], sg.c_end[i], sg.P[i], sg.kind[i] = c0, c1, P, kinds[i]
            sg.s[i], sg.q[i] = ts.data_ptr(), tq.data_ptr()
        beta_d = _cuda(beta)
        what = "finalize_segs integer=%s" % integer
        dbuf, dbeta = _guarded(C)
        cbuf, coef = _guarded(2 * C)
        ops.bn_bwd_finalize_segs(sg, M, C, beta_d, dbeta, coef)
        torch.cuda.synchronize()
        assert _guards_intact(dbuf) and _guards_intact(cbuf)
        _check_finalized(what, integer, M, s, q, abs_s, abs_q, _np(dbeta), _np(coef).reshape(2, C))
        # _multi: every segment a layer with its own beta / dbeta vector; the third layer's dbeta is not wanted
        betas = [beta_d[c0:c1].clone() for c0, c1 in zip(cuts[:-1], cuts[1:])]
        douts = [_guarded(c1 - c0) for c0, c1 in zip(cuts[:-1], cuts[1:])]
        cbuf2, coef2 = _guarded(2 * C)
        ops.bn_bwd_finalize_multi(sg, M, C, betas, [None if i == 2 else douts[i][1] for i in range(4)], coef2)
        torch.cuda.synchronize()
        assert _guards_intact(cbuf2) and all(_guards_intact(buf) for buf, _ in douts)
        assert bool((douts[2][1] == SENT).all())
        assert _same_bits(coef2, coef)
        for i, (c0, c1) in enumerate(zip(cuts[:-1], cuts[1:])):
            if i != 2:
                assert _same_bits(douts[i][1], dbeta[c0:c1])


# ---- 3. the apply family ----------------------------------------------------------------------------------------------------
def _amax_record():
    buf, rec = _guarded(_ops().AMAX_FLOATS, fill=0.0)
    buf[:GUARD] = SENT
    buf[-GUARD:] = SENT
    return buf, rec


def _check_amax(buf, rec, value):
    """The record's value (the maximum of its 16 slots) is `value`; nothing but the slots was written."""
    ops = _ops()
    assert _guards_intact(buf)
    assert bool((rec.view(16, 32)[:, 1:] == 0).all())
    assert ops.amax_value(rec) == float(value)


def _third_row_rule(M, C):
    """The long shape: the smallest M at which a thread of the launch walks a third row (2 * drow < M)."""
    ops = _ops()
    C4 = C // 4
    assert 2 * ops.bn_infer_bwd_partials(M, C) * 256 // C4 < M
    assert not 2 * ops.bn_infer_bwd_partials(M - 1, C) * 256 // C4 < M - 1


@pytest.mark.parametrize("shape", B.DENSE + B.WALK, ids=B.shape_id)
@pytest.mark.parametrize("mode", ["exact", "real"])
def test_apply_family_writes_the_references_dz(mode, shape):
    """ds_bn_bwd_apply out of place and in place (the same bits), _bf16 and _z16 into a bf16 tensor with lddz > C, the max|dz|
    record on and off, ds_bn_bwd_apply_cols on a middle segment: a missing second row, a third row (the long shape), C > 1024,
    z's columns >= C and every slack untouched."""
    ops = _ops()
    M, C, ldz, cuts = shape
    if M == B.LONG_M:
        _third_row_rule(M, C)
    # (the long shape is there for the third row: its real inputs are built once, with z on the bf16 grid, for every entry
    # point; z with a full fp32 significand goes through the seven other shapes)
    one_build = mode == "exact" or M == B.LONG_M
    b = B.build(mode, M, C, z_bf16=(M == B.LONG_M))
    ref = B.reference(b.z, b.dy, b.mean, b.rstd, b.shift, b.coef)
    d = Dev(b, shape, z16=one_build)
    name = "apply %s %s" % (mode, B.shape_id(shape))
    tol = B.elem_tol(ref) if mode == "real" else None

    def run(z, dz, amax=None, dd=d):
        ops.bn_bwd_apply(z, dd.segs, M, C, dd.mean, dd.rstd, dd.shift, dd.coef, dz, amax=amax, ldz=ldz)
        torch.cuda.synchronize()

    def check32(what, got):
        if mode == "exact":
            _bit_equal(what, got, ref.dz.astype(F32))
        else:
            _within(what, np.abs(got - ref.dz), tol)

    # fp32, out of place, with the record
    dz = torch.full((M, ldz), SENT, device="cuda")
    abuf, rec = _amax_record()
    run(d.z, dz, rec)
    d.assert_inputs_intact()
    assert bool((dz[:, C:] == SENT).all())
    got = _np(dz[:, :C])
    check32(name + " fp32", got)
    _check_amax(abuf, rec, np.abs(got).max())
    if mode == "exact":
        assert ops.amax_value(rec) == float(np.abs(ref.dz).max())
    # ... without the record: the same bits
    dz2 = torch.full((M, ldz), SENT, device="cuda")
    run(d.z, dz2)
    assert _same_bits(dz2, dz)
    # in place (both rows' loads stand ahead of the stores)
    zc = d.z.clone()
    run(zc, zc)
    d.assert_inputs_intact()
    assert _same_bits(zc[:, :C], dz[:, :C])
    assert bool(torch.isnan(zc[:, C:]).all())
    # bf16 out (lddz > C), from fp32 z and from bf16 z
    lddz = C + 8
    for z16 in (False, True):
        bb, rr, dd = b, ref, d
        if z16 and not one_build:                                         # z on the bf16 grid: a case of its own
            bb = B.build(mode, M, C, z_bf16=True)
            rr = B.reference(bb.z, bb.dy, bb.mean, bb.rstd, bb.shift, bb.coef)
            dd = Dev(bb, shape, z16=True)
        dz16 = torch.full((M, lddz), SENT16, dtype=torch.bfloat16, device="cuda")
        abuf16, rec16 = _amax_record()
        run(dd.z16 if z16 else dd.z, dz16, rec16, dd)
        dd.assert_inputs_intact()
        assert bool((dz16[:, C:] == SENT16).all())
        got16 = _np(dz16[:, :C])
        what = name + (" bf16 z -> bf16" if z16 else " fp32 z -> bf16")
        if mode == "exact":
            _bit_equal(what, got16, B.bf16_round(rr.dz.astype(F32)))
        else:
            _within(what, np.abs(got16 - rr.dz), B.elem_tol(rr) + B.bf16_ulp(rr.dz))
        # the record holds max|dz| before the rounding of the store, which is monotonic: its bf16 value is the tensor's
        # maximum, and it is the fp32 apply's record on the same z
        if dd is d:
            full_max = float(np.abs(got).max())
        else:
            full = torch.full((M, ldz), SENT, device="cuda")
            run(dd.z, full, None, dd)
            full_max = float(full[:, :C].abs().max())
        _check_amax(abuf16, rec16, full_max)
        assert float(B.bf16_round(F32(ops.amax_value(rec16)))) == float(np.abs(got16).max())
        if mode == "exact":
            assert ops.amax_value(rec16) == float(np.abs(rr.dz).max())
    # a column range of the layer over the shared z / dz buffer
    if len(cuts) > 2:
        c0, c1 = cuts[1], cuts[2]
        zc = d.z.clone()
        c0p, c1p, ptr, ld = d.parts[1]
        seg = ops.make_segments([(0, c1 - c0, ptr, ld)])
        ops.bn_bwd_apply_cols(zc[:, c0:], seg, M, c1 - c0, d.mean[c0:], d.rstd[c0:], d.shift[c0:], d.coef[0, c0:], d.coef[1, c0:],
                              zc[:, c0:], ldz)
        torch.cuda.synchronize()
        d.assert_inputs_intact()
        assert _same_bits(zc[:, c0:c1], dz[:, c0:c1])
        assert _same_bits(zc[:, :c0], d.z[:, :c0]) and _same_bits(zc[:, c1:], d.z[:, c1:])
        print("ANCHOR %s cols [%d, %d): the bits of the whole-layer apply" % (name, c0, c1))


# ---- 4. the chain -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", B.DENSE, ids=B.shape_id)
def test_chain_on_the_devices_own_coefficients(shape):
    """reduce -> finalize -> apply (in place) on real inputs: dbeta and coef inside the sums bound, dz inside the element bound
    plus the propagated error of the coefficients."""
    ops = _ops()
    M, C, ldz, cuts = shape
    b = B.build("real", M, C)
    ref = B.reference(b.z, b.dy, b.mean, b.rstd, b.shift)
    d = Dev(b, shape)
    n = B.dense_chain(M)
    P = ops.bn_bwd_partials(M, C)
    pbuf, part = _guarded(2 * C * P)
    dbuf, dbeta = _guarded(C)
    cbuf, coef = _guarded(2 * C)
    zc = d.z.clone()
    ops.bn_bwd_reduce(zc, d.segs, M, C, d.mean, d.rstd, d.shift, part, ldz=ldz)
    ops.bn_bwd_finalize(part, P, M, C, dbeta, coef)
    ops.bn_bwd_apply(zc, d.segs, M, C, d.mean, d.rstd, d.shift, coef, zc, ldz=ldz)
    torch.cuda.synchronize()
    d.assert_inputs_intact()
    assert _guards_intact(pbuf) and _guards_intact(dbuf) and _guards_intact(cbuf)
    assert bool(torch.isnan(zc[:, C:]).all())
    name = "chain %s" % B.shape_id(shape)
    co = _np(coef).reshape(2, C)
    _within(name + " dbeta", np.abs(_np(dbeta) - ref.S1), B.sums_tol(n, ref.A1))
    _within(name + " coef[0]", np.abs(co[0] - ref.coef[0]), B.sums_tol(n, ref.A1) / M)
    _within(name + " coef[1]", np.abs(co[1] - ref.coef[1]), B.sums_tol(n, ref.A2) / M)
    _within(name + " dz", np.abs(_np(zc[:, :C]) - ref.dz), B.elem_tol(ref) + B.chain_extra(ref, n))


def test_exact_chain_coefficients_are_within_one_ulp():
    """reduce -> finalize on exact inputs: dbeta has the reference's bits; coef = sum * (1 / M) in double, then one rounding,
    is at most one fp32 ulp from the reference's sum / M."""
    ops = _ops()
    for shape in B.DENSE:
        M, C, ldz, cuts = shape
        b = B.build("exact", M, C)
        ref = B.reference(b.z, b.dy, b.mean, b.rstd, b.shift)
        d = Dev(b, shape)
        P = ops.bn_bwd_partials(M, C)
        part = torch.empty(2 * C * P, device="cuda")
        dbuf, dbeta = _guarded(C)
        cbuf, coef = _guarded(2 * C)
        ops.bn_bwd_reduce(d.z, d.segs, M, C, d.mean, d.rstd, d.shift, part, ldz=ldz)
        ops.bn_bwd_finalize(part, P, M, C, dbeta, coef)
        torch.cuda.synchronize()
        assert _guards_intact(dbuf) and _guards_intact(cbuf)
        _bit_equal("exact chain %s dbeta" % B.shape_id(shape), _np(dbeta), ref.S1.astype(F32))
        apart = B.ulps_apart(_np(coef).reshape(2, C), ref.coef.astype(F32))
        print("ANCHOR exact chain %s coef: at most %d ulp from the reference" % (B.shape_id(shape), apart.max()))
        assert apart.max() <= 1


# ---- 5. the three spellings of the ReLU mask ----------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", B.KNIFE, ids=B.shape_id)
def test_every_pass_takes_the_fused_decision_on_knife_edge_elements(shape):
    """A quarter of every channel sits where fl(z * rstd) == -shift but z * rstd != -shift: an unfused fp32 predicate says 0
    there, the fused multiply-add says the sign of the residual, and so does fp64.  The forward pass, the reduce, the apply and
    the moving-statistics apply must all take the reference's decision, element by element (dy is a positive integer: every
    comparison is exact)."""
    ops = _ops()
    M, C, ldz, cuts = shape
    b = B.build("knife", M, C)
    ref = B.reference(b.z, b.dy, b.mean, b.rstd, b.shift)
    d = Dev(b, shape)
    name = "knife %s" % B.shape_id(shape)
    pos = b.knife & (b.knife_sign > 0)
    assert pos.any(0).all() and (b.knife & ~pos).any(0).all()

    def report(what, mask):
        wrong = mask != ref.mask
        print("ANCHOR %s %s: %d decisions differ from fp64 (%d on positive knife-edge elements of %d)"
              % (name, what, wrong.sum(), (wrong & pos).sum(), pos.sum()))
        return int(wrong.sum())

    # the activation the forward pass writes (dense z; the destination in the segments' layout)
    ys, yparts = [], []
    for i, (c0, c1) in enumerate(zip(cuts[:-1], cuts[1:])):
        ld = (c1 - c0) + 4 * (i + 1)
        t = torch.full((M, ld), SENT, device="cuda")
        ys.append(t)
        yparts.append((c0, c1, t.data_ptr(), ld))
    ops.bn_apply_relu(d.z[:, :C].contiguous(), M, C, d.rstd, d.shift, ops.make_segments(yparts))
    torch.cuda.synchronize()
    y = np.concatenate([_np(t[:, :c1 - c0]) for t, (c0, c1) in zip(ys, zip(cuts[:-1], cuts[1:]))], axis=1)
    assert all(bool((t[:, c1 - c0:] == SENT).all()) for t, (c0, c1) in zip(ys, zip(cuts[:-1], cuts[1:])))
    bad_fwd = report("forward y > 0", y > 0)
    # the apply with zero coefficients: dz = rstd * g
    zero = torch.zeros(2, C, device="cuda")
    dz = torch.full((M, ldz), SENT, device="cuda")
    ops.bn_bwd_apply(d.z, d.segs, M, C, d.mean, d.rstd, d.shift, zero, dz, ldz=ldz)
    torch.cuda.synchronize()
    got = _np(dz[:, :C])
    bad_apply = report("apply dz != 0", got != 0)
    # the moving-statistics apply
    dzi = torch.full((M, ldz), SENT, device="cuda")
    ops.bn_infer_bwd_apply(d.z, d.segs, M, C, d.rstd, d.shift, dzi, ldz=ldz)
    torch.cuda.synchronize()
    goti = _np(dzi[:, :C])
    bad_infer = report("moving-statistics apply dz != 0", goti != 0)
    # the reduce: sum g over the mask it took (integers)
    P = ops.bn_bwd_partials(M, C)
    pbuf, part = _guarded(2 * C * P)
    ops.bn_bwd_reduce(d.z, d.segs, M, C, d.mean, d.rstd, d.shift, part, ldz=ldz)
    torch.cuda.synchronize()
    sums = _partial_sums(part, C, P)
    unfused = np.where(ref.mask & ~pos, b.dy, 0).astype(np.float64).sum(0)
    print("ANCHOR %s reduce sum g: %d channels differ from fp64 (%d equal the sum an unfused predicate would give)"
          % (name, (sums[0] != ref.S1).sum(), (sums[0] == unfused).sum()))
    d.assert_inputs_intact()
    assert bad_fwd == 0 and bad_apply == 0 and bad_infer == 0
    assert np.array_equal(sums[0], ref.S1)
    want = (b.rstd.astype(np.float64) * ref.g).astype(F32)
    _bit_equal(name + " apply dz = rstd * g", got, want)
    _bit_equal(name + " moving-statistics apply dz = rstd * g", goti, want)
    _within(name + " sum g*xhat", np.abs(sums[1] - ref.S2), B.sums_tol(B.dense_chain(M), ref.A2))


# ---- 6. the pooled twins ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", B.POOLED, ids=lambda s: "%dx%dx%dx%d" % s)
@pytest.mark.parametrize("mode", ["exact", "real"])
def test_pooled_twins_follow_the_oracles_pool_gradient(mode, shape):
    """ds_bn_pool_bwd_reduce / _apply from the POOLED gradient and the winners of ops.maxpool_bn_relu_fwd, against the oracle's
    S.max_pool_bwd followed by the dense reference: exact bits, real bounds (|g| = the routed magnitudes), the chain on the
    device's coefficients, identical repeats, the in-place apply."""
    ops = _ops()
    N, H, W, C = shape
    p = B.build_pooled(mode, N, H, W, C)
    M, OH, OW = N * H * W, -(-H // 2), -(-W // 2)
    name = "pooled %s %dx%dx%dx%d" % ((mode,) + shape)
    z, dpool = _cuda(p.z4), _cuda(p.dpool)
    mean, rstd, shift, coef = _cuda(p.mean), _cuda(p.rstd), _cuda(p.shift), _cuda(p.coef)
    y = torch.empty(N, OH, OW, C, device="cuda")
    am = torch.empty(N, OH, OW, C, dtype=torch.uint8, device="cuda")
    assert ops.maxpool_bn_relu_fwd(z, rstd, shift, y, am, N, H, W, C, 3, 2) == (OH, OW)
    torch.cuda.synchronize()
    assert np.array_equal(am.cpu().numpy(), p.winners)
    z0, dpool0, am0 = z.clone(), dpool.clone(), am.clone()
    P = ops.bn_pool_bwd_partials(N, H, W, C)
    n = B.pooled_chain(p.patches, C // 4, P)
    own = B.reference(p.z, p.dy, p.mean, p.rstd, p.shift, g_mag=p.dy_mag)
    parts = []
    for _ in range(2):
        pbuf, part = _guarded(2 * C * P)
        ops.bn_pool_bwd_reduce(z, dpool, am, N, H, W, C, mean, rstd, shift, part)
        torch.cuda.synchronize()
        assert _guards_intact(pbuf) and bool((part != SENT).all())
        parts.append(part)
    assert _same_bits(parts[0], parts[1])
    sums = _partial_sums(parts[0], C, P)
    if mode == "exact":
        _bit_equal(name + " sum g", sums[0].astype(F32), own.S1.astype(F32))
        _bit_equal(name + " sum g*xhat", sums[1].astype(F32), own.S2.astype(F32))
        assert np.array_equal(sums[0], own.S1) and np.array_equal(sums[1], own.S2)
    else:
        _within(name + " sum g", np.abs(sums[0] - own.S1), B.sums_tol(n, own.A1))
        _within(name + " sum g*xhat", np.abs(sums[1] - own.S2), B.sums_tol(n, own.A2))
    # the apply on given coefficients, out of place and in place
    ref = B.reference(p.z, p.dy, p.mean, p.rstd, p.shift, p.coef, g_mag=p.dy_mag)
    dbuf, dzf = _guarded(M * C)
    dz = dzf.view(N, H, W, C)
    ops.bn_pool_bwd_apply(z, dpool, am, N, H, W, C, mean, rstd, shift, coef, dz)
    zc = z.clone()
    ops.bn_pool_bwd_apply(zc, dpool, am, N, H, W, C, mean, rstd, shift, coef, zc)
    torch.cuda.synchronize()
    assert _guards_intact(dbuf) and _same_bits(zc, dz)
    got = _np(dz).reshape(M, C)
    if mode == "exact":
        _bit_equal(name + " dz", got, ref.dz.astype(F32))
    else:
        _within(name + " dz", np.abs(got - ref.dz), B.elem_tol(ref))
        # the chain: the device's own coefficients
        cbuf, cdev = _guarded(2 * C)
        bbuf, dbeta = _guarded(C)
        ops.bn_bwd_finalize(parts[0], P, M, C, dbeta, cdev)
        zc = z.clone()
        ops.bn_pool_bwd_apply(zc, dpool, am, N, H, W, C, mean, rstd, shift, cdev, zc)
        torch.cuda.synchronize()
        assert _guards_intact(cbuf) and _guards_intact(bbuf)
        _within(name + " chain dbeta", np.abs(_np(dbeta) - own.S1), B.sums_tol(n, own.A1))
        _within(name + " chain dz", np.abs(_np(zc).reshape(M, C) - own.dz), B.elem_tol(own) + B.chain_extra(own, n))
    assert _same_bits(z, z0) and _same_bits(dpool, dpool0) and torch.equal(am, am0)


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------
def test_refused_calls_return_an_error_and_launch_nothing():
    ops = _ops()
    M, C = 8, 16
    wide = 1032
    z = torch.zeros(M, wide, device="cuda")
    z16 = torch.zeros(M, C, dtype=torch.bfloat16, device="cuda")
    dy = torch.ones(M, wide, device="cuda")
    vec = torch.ones(wide + 4, device="cuda")
    coef = torch.zeros(2, C, device="cuda")
    part = torch.full((2 * wide * 8,), SENT, device="cuda")
    dbeta = torch.full((C,), SENT, device="cuda")
    cout = torch.full((2 * C,), SENT, device="cuda")
    raw = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)

    def segs(c1, ld=wide, dtype=None):
        e = (0, c1, dy.data_ptr(), ld)
        return ops.make_segments([e if dtype is None else e + (dtype,)])

    sg = ops.SumSegments()
    sg.nseg = 1
    sg.c_begin[0], sg.c_end[0], sg.P[0], sg.kind[0] = 0, C, 8, 1
    sg.s[0], sg.q[0] = part.data_ptr(), part.data_ptr() + 4 * C * 8
    bad = [lambda: ops.bn_bwd_reduce(z, segs(1028), M, 1028, vec, vec, vec, part, ldz=wide),                     # C > 1024
           lambda: ops.bn_bwd_reduce(z, segs(6), M, 6, vec, vec, vec, part, ldz=wide),                           # C % 4
           lambda: ops.bn_bwd_reduce(z, segs(C), M, C, vec, vec, vec, part, ldz=12),                             # ldz < C
           lambda: ops.bn_bwd_reduce(raw(z), segs(C), M, C, raw(vec, 4), raw(vec), raw(vec), raw(part), ldz=wide),  # mean + 4 bytes
           lambda: ops.bn_bwd_reduce(z, segs(C - 4), M, C, vec, vec, vec, part, ldz=wide),                       # C - 4 covered
           lambda: ops.bn_bwd_reduce(z, segs(C, dtype=ops.DS_DTYPE_BF16), M, C, vec, vec, vec, part, ldz=wide),  # bf16 segment
           lambda: ops.bn_bwd_reduce(raw(z), segs(C), M, C, raw(vec), raw(vec), raw(vec), raw(part), ldz=wide, z_dtype=99),
           lambda: ops.bn_bwd_apply(z16, segs(C), M, C, vec, vec, vec, coef, z16, ldz=C),                        # dz16 == z16
           lambda: ops.bn_bwd_finalize_segs(sg, M, C, None, dbeta, cout)]                                        # kind 1, no beta
    z16_0 = z16.clone()
    for i, call in enumerate(bad):
        with pytest.raises(RuntimeError):
            call()
        torch.cuda.synchronize()
        assert bool((part == SENT).all()) and bool((dbeta == SENT).all()) and bool((cout == SENT).all()), i
        assert _same_bits(z16, z16_0) and bool((z == 0).all()), i
    # (the same calls with the defect removed go through)
    ops.bn_bwd_reduce(z, segs(C), M, C, vec, vec, vec, part, ldz=wide)
    torch.cuda.synchronize()
    assert bool((part[:2 * C * ops.bn_bwd_partials(M, C)] != SENT).all())
