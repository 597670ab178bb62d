"""The BatchNorm forward kernels of csrc/bn.hip against fp64 at their edges: ds_bn_finalize, ds_bn_finalize_centered,
ds_bn_finalize_multi, ds_bn_apply_relu, ds_bn_apply_relu_z16, ds_bn_infer_prepare and ds_bn_infer_prepare_multi.  Reference,
derived gates, case tables and the checks themselves: tests/bn_fwd_ref.py (proved neither vacuous nor too tight by
tests/test_bn_fwd_ref_cpu.py).  Every output lives in a buffer of this module with sentinel guards on both sides and sentinels
in every column no segment owns; inputs are compared with their copies after every launch.  The last test prints, per entry
point, the largest error / gate of every check."""
import numpy as np
import pytest
import torch

import bn_fwd_ref as R

pytestmark = pytest.mark.gpu

F32 = np.float32
GUARD = R.GUARD
WORST = R.Report()


def _ops():
    from tumblr_emotions_amd import ops
    assert (ops.DS_DTYPE_F32, ops.DS_DTYPE_BF16, ops.AMAX_FLOATS) == (R.DT_F32, R.DT_BF16, R.AMAX_FLOATS)
    return ops


def _cuda(a, dtype=torch.float32):
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


def _guarded(n, fill=R.SENT, dtype=torch.float32):
    """A tensor of n elements between two guards of sentinels: (whole buffer, view of the n elements)."""
    buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device="cuda")
    return buf, buf[GUARD:GUARD + n]


def _guards_intact(buf, fill=R.SENT):
    return bool((buf[:GUARD] == fill).all()) and bool((buf[-GUARD:] == fill).all())


def _bits(t):
    t = t.contiguous()
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _np(t):
    return t.float().cpu().numpy()


# ---- 1. finalize ----------------------------------------------------------------------------------------------------------------
def _finalize_outputs(k, moving, centered):
    names = ["mean", "rstd", "shift"] + (["mean_c", "shift_c"] if centered else []) + \
        (["mm"] if moving[0] else []) + (["mv"] if moving[1] else [])
    out = {n: _guarded(k.C) for n in names}
    if "mm" in out:
        out["mm"][1].copy_(_cuda(k.mm0))
    if "mv" in out:
        out["mv"][1].copy_(_cuda(k.mv0))
    return out


def _launch_finalize(k, decay, moving, centered):
    """One single-layer launch of the case's partials; returns the outputs as host arrays after the containment checks."""
    ops = _ops()
    stats, beta = _cuda(k.stats), _cuda(k.beta)
    keep = [(stats, stats.clone()), (beta, beta.clone())]
    out = _finalize_outputs(k, moving, centered)
    pivot = None
    if k.pivot_kind == "alias":          # the pivot IS the mean vector (the previous step's mean): read before the write
        out["mean"][1].copy_(_cuda(k.pivot))
        pivot = out["mean"][1]
    elif k.pivot_kind == "sep":
        pivot = _cuda(k.pivot)
        keep.append((pivot, pivot.clone()))
    v = lambda n: out[n][1] if n in out else None
    if centered:
        ops.bn_finalize_centered(stats, k.P, k.count, k.C, beta, float(k.eps), float(decay), v("mean"), v("rstd"), v("shift"),
                                 v("mm"), v("mv"), pivot, v("mean_c"), v("shift_c"))
    else:
        ops.bn_finalize(stats, k.P, k.count, k.C, beta, float(k.eps), float(decay), v("mean"), v("rstd"), v("shift"), v("mm"),
                        v("mv"), pivot=pivot)
    torch.cuda.synchronize()
    for n, (buf, view) in out.items():
        assert _guards_intact(buf), n
    for t, t0 in keep:
        assert _same_bits(t, t0)
    return {n: _np(view).astype(F32) for n, (_, view) in out.items()}


@pytest.mark.parametrize("case", R.FINALIZE, ids=R.fin_id)
def test_finalize_against_fp64(case):
    """ds_bn_finalize / ds_bn_finalize_centered from fp32 partials [2][C][P] of a real z.  P = 1, 63, 64 leave waves idle or
    exactly full; 255 / 256 fill the one trip of finalize_channel's strided loop; 257, 700 and 2048 (the product's largest)
    take 2, 3 and 8 trips of `p += 256`, each with no pivot, a separate pivot and a pivot that aliases mean (read before
    write).  C = 4 / 176 / 1024 workgroups; count = P (one row per partial), 3000, 256*112*112.  Channels with |mean| = 50
    sigma, a constant channel, and a channel whose q/count - du^2 is slightly negative: the var < 0 clamp gives
    rstd = 1/sqrt(eps) and a batch variance of 0.  The four null / non-null combinations of the moving vectors; decay 0.9997
    and 0.  A second launch with decay 0 exposes the kernel's fp32 cast of var (mv <- var) and must repeat mean, rstd and
    shift bit for bit."""
    k = R.build_finalize(*case)
    got = _launch_finalize(k, k.decay, k.moving, k.centered)
    probe = _launch_finalize(k, F32(0), (True, True), k.centered)
    rep = R.check_finalize(k, got, probe, what="ds_bn_finalize_centered" if k.centered else "ds_bn_finalize")
    WORST.merge(rep)


# ---- 2. finalize_multi ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("jobs", R.FINALIZE_MULTI, ids=lambda j: "%djobs" % len(j[1]))
def test_finalize_multi_against_fp64_and_the_single_launches(jobs):
    """ds_bn_finalize_multi with 1, 2, 3 and 4 jobs of different C, P and count: the workgroup -> job search over `first[]`
    with C = 4 beside C = 832, P = 1 beside P = 700 / 2048 (a job whose strided loop makes no full trip beside one that makes
    eight), a job without moving vectors beside one with them (independently null), and pivots that alias the job's slice
    of ONE concatenated mean vector.  Every job passes the fp64 gates and equals its single launch bit for bit."""
    ops = _ops()
    decay, js = jobs
    ks = [R.build_finalize(*j, decay=decay, seed=10 + i) for i, j in enumerate(js)]
    total = sum(k.C for k in ks)
    mean_buf, mean_cat = _guarded(total)
    outs, launch, keep, c0 = [], [], [], 0
    for k in ks:
        out = _finalize_outputs(k, k.moving, False)
        out["mean"] = (mean_buf, mean_cat[c0:c0 + k.C])
        c0 += k.C
        stats, beta = _cuda(k.stats), _cuda(k.beta)
        keep += [(stats, stats.clone()), (beta, beta.clone())]
        pivot = None
        if k.pivot_kind == "alias":
            out["mean"][1].copy_(_cuda(k.pivot))
            pivot = out["mean"][1]
        elif k.pivot_kind == "sep":
            pivot = _cuda(k.pivot)
            keep.append((pivot, pivot.clone()))
        v = lambda n, out=out: out[n][1] if n in out else None
        launch.append((stats, k.P, k.count, k.C, beta, pivot, v("mean"), v("rstd"), v("shift"), v("mm"), v("mv")))
        outs.append(out)
    ops.BnFinalizeJobs(launch).run(float(R.EPS), float(decay))
    torch.cuda.synchronize()
    for t, t0 in keep:
        assert _same_bits(t, t0)
    for k, out in zip(ks, outs):
        for n, (buf, view) in out.items():
            assert _guards_intact(buf), n
        got = {n: _np(view).astype(F32) for n, (_, view) in out.items()}
        single = _launch_finalize(k, decay, k.moving, False)
        for n in got:
            assert np.array_equal(got[n].view(np.uint32), single[n].view(np.uint32)), n
        probe = _launch_finalize(k, F32(0), (True, True), False)
        WORST.merge(R.check_finalize(k, got, probe, what="ds_bn_finalize_multi"))


# ---- 3. apply ---------------------------------------------------------------------------------------------------------------------
def _launch_apply(k):
    """ds_bn_apply_relu (z fp32) or ds_bn_apply_relu_z16 (z bf16) into the case's segment layout: (destination tensors as
    float32 [M, ld] host arrays, per segment its record's words or None)."""
    ops = _ops()
    z = _cuda(k.z)
    if k.z16:
        z = z.to(torch.bfloat16)
        assert np.array_equal(_np(z), k.z)                     # z is read back exactly
    z0 = z.clone()
    rstd, shift = _cuda(k.rstd), _cuda(k.shift)
    bufs = [_guarded(k.M * ld, R.SENT if dt == R.DT_F32 else R.SENT16, torch.float32 if dt == R.DT_F32 else torch.bfloat16)
            for ld, dt in k.buffers]
    recs, entries = [], []
    for (c0, c1, bi, col, has_rec, _) in k.segs:
        ld, dt = k.buffers[bi]
        view = bufs[bi][1]
        rec = None
        if has_rec:
            rec = _guarded(R.AMAX_FLOATS)
            rec[1][::32] = 0
        recs.append(rec)
        entries.append((c0, c1, view.data_ptr() + col * view.element_size(), ld, dt, rec[1].data_ptr() if rec else None))
    ops.bn_apply_relu(z, k.M, k.C, rstd, shift, ops.make_segments(entries))
    torch.cuda.synchronize()
    assert _same_bits(z, z0) and np.array_equal(_np(rstd), k.rstd) and np.array_equal(_np(shift), k.shift)
    for (buf, _), (ld, dt) in zip(bufs, k.buffers):
        assert _guards_intact(buf, R.SENT if dt == R.DT_F32 else R.SENT16)
    for rec in recs:
        assert rec is None or _guards_intact(rec[0])
    return ([_np(view).reshape(k.M, ld) for (_, view), (ld, _) in zip(bufs, k.buffers)],
            [None if rec is None else _np(rec[1]) for rec in recs])


def _assert_reach(shape):
    """The restated launch rule is the library's (ds_bn_infer_bwd_partials answers with column_grid's grid), and the two long
    cases walk three rows or more per thread: a second pass of `row += NR * drow`."""
    M, C = shape
    assert _ops().bn_infer_bwd_partials(M, C) == R.column_grid(M, C)[0]
    most, fewest = R.rows_per_thread(M, C)
    if shape == R.LONG_ONE_ROW_TAIL:
        assert (most, fewest) == (3, 2)          # the threads that make a second pass have no second row in it (ok[1] false)
    if shape == R.LONG_SOME_ROWS_TAIL:
        assert (most, fewest) == (4, 3)          # every thread makes a second pass, only some with a second row


@pytest.mark.parametrize("shape", R.APPLY, ids=R.apply_id)
def test_apply_relu_against_fp64(shape):
    """ds_bn_apply_relu, y = max(z rstd + shift, 0) into column segments.  1 x 4: one thread with work (M = 1 < drow = 256).
    1 x 1024: one row across a whole workgroup, four segments given out of channel order, cuts inside a wave, records on two
    segments only (the per-segment wave reduction with `sgi != i` lanes), one all-negative segment whose record stays 0.
    7 x 12 (M < drow: most threads have no row), 255 x 1000 (a record on one side of a cut that halves every second wave),
    1001 x 832, 777 x 176: grid granules C4 / gcd(C4, 256) = 3, 125, 13, 11; fp32 and bf16 destinations mixed in one call; the
    64 | 96 | 16 split with two slices inside one wider concat row (ld > width).  140001 x 64 and 196685 x 64: the capped grid,
    so `row += NR * drow` makes a second pass -- without a second row (`ok[1]` false, the load falls back to `row`) for every
    thread, or for all but the first 77 rows.  z holds exact zeros, values within an ulp of the ReLU kink, and values whose
    z rstd + shift is exactly halfway between two bf16 numbers (round to nearest EVEN)."""
    _assert_reach(shape)
    k = R.build_apply(*shape)
    WORST.merge(R.check_apply(k, *_launch_apply(k), what="ds_bn_apply_relu"))


@pytest.mark.parametrize("shape", R.APPLY_Z16, ids=R.apply_id)
def test_apply_relu_z16_against_fp64(shape):
    """ds_bn_apply_relu_z16: the same launches (the 50 MB one excepted) reading z from bf16 storage -- 8-byte loads, the
    widening on load, the same row walk and segment scatter."""
    _assert_reach(shape)
    k = R.build_apply(*shape, z16=True)
    WORST.merge(R.check_apply(k, *_launch_apply(k), what="ds_bn_apply_relu_z16"))


# ---- 5. the bit-identity the other tests lean on ----------------------------------------------------------------------------------
def _apply_dense(z, M, C, rstd, shift, cuts, dt):
    """A launch over the first M rows of z into one tensor per segment (cuts), returned as one [M, C] tensor."""
    ops = _ops()
    tdt = torch.float32 if dt == R.DT_F32 else torch.bfloat16
    outs, entries = [], []
    for c0, c1 in zip(cuts[:-1], cuts[1:]):
        buf, view = _guarded(M * (c1 - c0), R.SENT if dt == R.DT_F32 else R.SENT16, tdt)
        outs.append((buf, view.view(M, c1 - c0)))
        entries.append((c0, c1, view.data_ptr(), c1 - c0, dt))
    ops.bn_apply_relu(z, M, C, rstd, shift, ops.make_segments(entries))
    torch.cuda.synchronize()
    for buf, _ in outs:
        assert _guards_intact(buf, R.SENT if dt == R.DT_F32 else R.SENT16)
    return torch.cat([v for _, v in outs], dim=1)


@pytest.mark.parametrize("dt", [R.DT_F32, R.DT_BF16], ids=["fp32", "bf16"])
def test_apply_relu_bits_do_not_depend_on_the_launch(dt):
    """What the wide-kernel, pool-on-load and fused-inference twins assume when they call ds_bn_apply_relu "the materialised
    form": an element's bits depend on (z, rstd, shift) alone -- not on M (rows [0, 300) of the 777-row launch against a
    300-row launch: another grid, another drow, another thread per element) and not on the segment split (one segment
    against four)."""
    k = R.build_apply(777, 176)
    z, rstd, shift = _cuda(k.z), _cuda(k.rstd), _cuda(k.shift)
    M1 = 300
    assert R.column_grid(777, 176) != R.column_grid(M1, 176)
    whole = _apply_dense(z, 777, 176, rstd, shift, (0, 176), dt)
    prefix = _apply_dense(z, M1, 176, rstd, shift, (0, 176), dt)
    four = _apply_dense(z, 777, 176, rstd, shift, (0, 64, 100, 160, 176), dt)
    assert _same_bits(whole[:M1], prefix)
    assert _same_bits(whole, four)
    assert float(whole.float().max()) > 0


# ---- 4. infer prepare -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", R.INFER_C)
def test_infer_prepare_against_fp64(C):
    """ds_bn_infer_prepare: C = 1 and 4 (one partly filled workgroup), 255 / 256 / 257 (the `c < C` edge on either side of a
    workgroup), 832, 1024; moving_var of 0 and near 0 (rstd at 1 / sqrt(eps)) up to 1e6."""
    ops = _ops()
    k = R.build_infer(C)
    ins = [_cuda(a) for a in (k.beta, k.mm, k.mv)]
    ins0 = [t.clone() for t in ins]
    (rb, r), (sb, s) = _guarded(C), _guarded(C)
    ops.bn_infer_prepare(ins[0], ins[1], ins[2], float(k.eps), C, r, s)
    torch.cuda.synchronize()
    assert _guards_intact(rb) and _guards_intact(sb) and all(_same_bits(a, b) for a, b in zip(ins, ins0))
    WORST.merge(R.check_infer(k, _np(r), _np(s), what="ds_bn_infer_prepare"))


class _Pool:
    """The vectors of many jobs in one tensor, a guard of sentinels before, between and after them."""

    def __init__(self, sizes, arrays=None):
        self.off = np.cumsum([GUARD] + [n + GUARD for n in sizes])[:-1]
        self.sizes = sizes
        self.t = torch.full((int(self.off[-1] + sizes[-1] + GUARD),), R.SENT, dtype=torch.float32, device="cuda")
        self.inside = torch.zeros_like(self.t, dtype=torch.bool)
        for j, n in enumerate(sizes):
            self.inside[self.off[j]:self.off[j] + n] = True
            if arrays is not None:
                self.view(j).copy_(_cuda(arrays[j]))

    def view(self, j):
        return self.t[int(self.off[j]):int(self.off[j]) + self.sizes[j]]

    def guards_intact(self):
        return bool((self.t[~self.inside] == R.SENT).all())


@pytest.mark.parametrize("njobs", R.INFER_MULTI)
def test_infer_prepare_multi_against_fp64_and_the_single_form(njobs):
    """ds_bn_infer_prepare_multi with 1, 57 (the tower), 64 (one full launch), 65 (the host loop's second launch holds one
    job) and 130 jobs (three launches), C of 1 .. 1024 mixed, so every launch has jobs narrower than its cmax whose
    blockIdx.y chunks must write nothing.  Every vector sits between guards; rstd / shift pass the fp64 gates and equal the
    single form's bits."""
    ops = _ops()
    Cs = R.infer_multi_jobs(njobs)
    ks = [R.build_infer(C, seed=j) for j, C in enumerate(Cs)]
    beta, mm, mv = (_Pool(Cs, [getattr(k, n) for k in ks]) for n in ("beta", "mm", "mv"))
    before = [p.t.clone() for p in (beta, mm, mv)]
    rstd, shift, rstd1, shift1 = (_Pool(Cs) for _ in range(4))
    ops.BnInferJobs([(beta.view(j), mm.view(j), mv.view(j), Cs[j], rstd.view(j), shift.view(j)) for j in range(njobs)]).run(
        float(R.EPS))
    for j in range(njobs):
        ops.bn_infer_prepare(beta.view(j), mm.view(j), mv.view(j), float(R.EPS), Cs[j], rstd1.view(j), shift1.view(j))
    torch.cuda.synchronize()
    assert all(_same_bits(p.t, b) for p, b in zip((beta, mm, mv), before))
    assert rstd.guards_intact() and shift.guards_intact() and rstd1.guards_intact() and shift1.guards_intact()
    assert torch.equal(rstd.t, rstd1.t) and torch.equal(shift.t, shift1.t)
    assert _same_bits(rstd.t, rstd1.t) and _same_bits(shift.t, shift1.t)
    for j, k in enumerate(ks):
        WORST.merge(R.check_infer(k, _np(rstd.view(j)), _np(shift.view(j)), what="ds_bn_infer_prepare_multi"))


# ---- the table ----------------------------------------------------------------------------------------------------------------------
def test_zz_report_worst_error_over_gate(capsys):
    """Prints what the tests above measured (nothing when they were deselected): entry point, check, largest error / gate."""
    with capsys.disabled():
        print("\nBatchNorm forward, largest error / gate per entry point and check:\n" + WORST.table())
    assert not WORST.failed()
