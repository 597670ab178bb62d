"""The fp64 reference, the gates and the case tables of tests/test_bn_fwd_gpu.py, checked on their own (no GPU): the reference
is the oracle's BatchNorm, a NumPy fp32 emulation of every kernel expression passes every gate of every case in either
contraction form (mul then add, or one fused multiply-add), every planted defect fails a gate on the smallest case that has
the code path, and the restated launch rule of the streaming kernels gives the hand-computed grids."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

import bn_fwd_ref as R
from conv_check import bf16_round
from oracle import tf_semantics as S

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMS = ("mul_add", "fma", "fma2")          # fma: the first product is the fused one; fma2: the second (moving updates)


# ---- NumPy emulations of the kernels ----------------------------------------------------------------------------------------------
def _f64(a):
    return np.asarray(a, np.float64)


def _nudge_ulps(a, n):
    return (np.asarray(a, F32).view(np.int32) + np.int32(n)).view(F32)


def _shift(beta, m32, r32, form):
    if form == "mul_add":
        return F32(beta) - F32(m32) * F32(r32)
    return (_f64(beta) - _f64(m32) * _f64(r32)).astype(F32)


def _moving(decay, old, batch32, form):
    d, omd = F32(decay), F32(1) - F32(decay)
    if form == "mul_add":
        return d * F32(old) + omd * F32(batch32)
    if form == "fma":
        return (float(d) * _f64(old) + _f64(omd * F32(batch32))).astype(F32)
    return (_f64(d * F32(old)) + float(omd) * _f64(batch32)).astype(F32)


def emulate_finalize(k, form, decay, moving, plant=None):
    st = k.stats.astype(np.float64)
    if plant == "last partial dropped":
        st = st[:, :, :-1]
    if plant == "second stride trip dropped":
        st = np.concatenate([st[:, :, :256], st[:, :, 512:]], axis=2)
    s, q = st[0].sum(axis=1), st[1].sum(axis=1)
    pv = 0.0 if k.pivot is None else _f64(k.pivot)
    du = s / k.count
    mu = du + (2 * pv if plant == "pivot added twice" else pv)
    var = q / k.count - du * du
    if plant == "unbiased variance":
        var = var * k.count / (k.count - 1)
    var = np.maximum(var, 0.0)
    r = (1.0 / np.sqrt(var + float(k.eps))).astype(F32)
    if plant == "rstd off by 4 ulps":
        r = _nudge_ulps(r, 4)
    mean = (du if plant == "mean_c taken for mean" else mu).astype(F32)
    out = {"mean": mean, "rstd": r, "shift": _shift(k.beta, mean, r, form)}
    if k.centered:
        out["mean_c"] = du.astype(F32)
        out["shift_c"] = _shift(k.beta, out["mean_c"], r, form)
    if moving[0]:
        out["mm"] = _moving(decay, k.mm0, mean, form)
    if moving[1]:
        out["mv"] = _moving(decay, k.mv0, var.astype(F32), form)
    return out


def run_finalize(k, form, plant=None):
    got = emulate_finalize(k, form, k.decay, k.moving, plant)
    probe = emulate_finalize(k, form, F32(0), (True, True), plant)
    return R.check_finalize(k, got, probe)


def emulate_apply(k, form, plant=None):
    z, r, s = k.z, k.rstd, k.shift
    if form == "mul_add":
        y = np.maximum(z * r + s, F32(0))
    else:
        y = np.maximum((z.astype(np.float64) * r.astype(np.float64) + s.astype(np.float64)).astype(F32), F32(0))
    assert y.dtype == F32
    if plant == "stale row in the second pass":
        _, drow = R.column_grid(k.M, k.C)
        assert k.M > 2 * drow
        y = y.copy()
        y[2 * drow:] = y[:k.M - 2 * drow]          # the pass's rows computed from the registers of the pass before
    bufs, recs = R.empty_buffers(k)
    for i, (c0, c1, bi, col, has_rec, _) in enumerate(k.segs):
        block = y[:, c0:c1]
        if k.buffers[bi][1] == R.DT_BF16:
            if plant == "truncation to bf16":
                block16 = (np.ascontiguousarray(block).view(np.uint32) & np.uint32(0xFFFF0000)).view(F32)
            else:
                block16 = bf16_round(block).astype(F32)
            bufs[bi][:, col:col + c1 - c0] = block16
        else:
            bufs[bi][:, col:col + c1 - c0] = block
        if has_rec:
            recs[i][0] = max(float(block.max()), 0.0)
    if plant == "column group in the neighbouring segment":
        # the first column group of the launch's second segment takes the first segment's pointer and stride
        (a0, a1, ab, acol, _, _), (b0, b1, bb, bcol, _, _) = k.segs[0], k.segs[1]
        bufs[bb][:, bcol:bcol + 4] = R.SENT if k.buffers[bb][1] == R.DT_F32 else R.SENT16
        flat = bufs[ab].reshape(-1)
        for row in range(k.M):
            e = row * k.buffers[ab][0] + acol + (b0 - a0)
            if 0 <= e and e + 4 <= flat.size:
                flat[e:e + 4] = y[row, b0:b0 + 4]
    return bufs, recs


def emulate_infer(k, form, plant=None):
    a = F32(k.mv) + F32(k.eps)
    sq = np.sqrt(a)
    assert sq.dtype == F32
    if plant == "sqrtf faithful, not nearest":      # the fp32 neighbour on the other side of the root: an error below 1 ulp
        sq = np.where(sq.astype(np.float64) > np.sqrt(a.astype(np.float64)), _nudge_ulps(sq, -1), _nudge_ulps(sq, 1))
    r = F32(1) / sq
    if plant == "rstd off by 4 ulps":
        r = _nudge_ulps(r, 4)
    return r, _shift(k.beta, k.mm, r, form)


def smallest(cases, build, has_path):
    """The smallest case (fewest elements) of a table that has the code path of a planted defect."""
    ks = [build(c) for c in cases]
    ks = [k for k in ks if has_path(k)]
    return min(ks, key=lambda k: k.size)


def _fin(c):
    k = R.build_finalize(*c)
    k.size = k.count * k.C
    return k


def _app(c):
    k = R.build_apply(*c)
    k.size = k.M * k.C
    return k


# ---- the reference ------------------------------------------------------------------------------------------------------------------
def test_reference_is_the_oracles_batch_norm():
    """Integer z: the fp32 partials are exact, so the finalize reference must give the oracle's mean / var / rstd / y and the
    oracle's moving update whatever the pivot and the chunking; the apply and infer references are the oracle's formulas."""
    rng = np.random.RandomState(3)
    count, C = 1000, 8
    z = rng.randint(-8, 9, size=(count, C)).astype(np.float64)
    beta = rng.normal(size=C)
    y, mean, var, _, rstd = S.batch_norm_train(z, beta)
    for P, pivot in ((1, None), (7, np.arange(C) - 3.0), (1000, np.full(C, 2.0))):
        u = z - (0 if pivot is None else pivot)
        cuts = np.arange(P) * count // P
        stats = np.stack([np.add.reduceat(u, cuts, axis=0).T, np.add.reduceat(u * u, cuts, axis=0).T]).astype(F32)
        ref = R.finalize_ref(stats, count, None if pivot is None else pivot.astype(F32), beta.astype(F32), R.EPS)
        assert np.abs(ref.mu - mean).max() <= 1e-13 and np.abs(ref.var - var).max() <= 1e-12
        want_r = 1.0 / np.sqrt(var + float(R.EPS))
        assert np.abs(ref.rstd - want_r).max() <= 1e-13 * want_r.max()
        assert np.abs(z * ref.rstd + ref.shift - (z - mean) * want_r - beta.astype(F32)).max() <= 1e-11
        if pivot is not None:
            assert np.abs(u * ref.rstd + ref.shift_c - (z * ref.rstd + ref.shift)).max() <= 1e-11
    assert abs(float(R.EPS) - S.BN_EPS) < 1e-10 and abs(float(R.DECAY) - S.BN_DECAY) < 1e-7
    assert abs(np.abs(y).max()) > 0
    k = R.build_infer(257)
    want = S.batch_norm_infer(np.ones(257), k.beta.astype(np.float64), k.mm.astype(np.float64), k.mv.astype(np.float64),
                              float(R.EPS))
    t, _ = R.shift_gate(k.beta, k.mm, k.r_ref.astype(F32))
    assert np.abs(k.r_ref + (k.beta - k.mm.astype(np.float64) * k.r_ref) - want).max() <= 1e-9 * np.abs(want).max()
    assert np.isfinite(t).all()


def test_the_gates_rest_on_the_flags_of_the_build():
    """infer_rstd_gate takes sqrtf at 1 ulp and the division as correctly rounded: true of the default fp32 code generation,
    which the library's compile line (csrc/Makefile, run by build()) must not switch off."""
    mk = open(os.path.join(ROOT, "tumblr_emotions_amd", "csrc", "Makefile")).read()
    flags = [l for l in mk.splitlines() if l.startswith("FLAGS")]
    assert len(flags) == 1 and "-O3" in flags[0]
    for banned in ("fast-math", "-fno-hip-fp32-correctly-rounded-divide-sqrt", "flush-denormals", "-Ofast", "unsafe-math",
                   "-ffp-contract", "approx-func", "reciprocal-math"):
        assert banned not in mk, banned
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert '"make", "-C", csrc' in entry
    assert R.SQRTF_ULP == 1.0 and R.DIVIDE_ULP == 0.5


def test_column_grid_restatement_against_hand_computed_launches():
    #            M,      C:   grid, drow, most / fewest rows of a thread
    want = {(1, 4): (1, 256, 1, 1),
            (1, 1024): (1, 1, 1, 1),
            (7, 12): (3, 256, 1, 1),
            (255, 1000): (125, 128, 2, 1),
            (1001, 832): (416, 512, 2, 1),
            (777, 176): (77, 448, 2, 1),
            (140001, 64): (4096, 65536, 3, 2),
            (196685, 64): (4096, 65536, 4, 3)}
    assert sorted(want) == sorted(R.APPLY)
    for (M, C), (grid, drow, most, fewest) in want.items():
        assert R.column_grid(M, C) == (grid, drow), (M, C)
        assert R.rows_per_thread(M, C) == (most, fewest), (M, C)
        C4 = C // 4
        assert grid % (C4 // math.gcd(C4, 256)) == 0 and grid <= R.KCUS * R.BPC + C4
    assert [math.gcd(c // 4, 256) for c in (4, 12, 832, 1000, 1024)] == [1, 1, 16, 2, 256]
    # the two long cases: every thread of a second pass is without a second row / only the rows below 77 have one
    M, C = R.LONG_ONE_ROW_TAIL
    drow = R.column_grid(M, C)[1]
    assert 2 * drow < M <= 3 * drow and M - 2 * drow == 8929
    M, C = R.LONG_SOME_ROWS_TAIL
    assert 3 * drow < M < 4 * drow and M - 3 * drow == 77
    assert M * C * 4 <= 51e6
    # the cap: a granule that does not divide it rounds the grid UP
    assert R.column_grid(10 ** 6, 1000) == (4125, 4224)


def test_case_tables_hold_what_the_issue_lists():
    Ps = {c[0] for c in R.FINALIZE}
    assert Ps == {1, 63, 64, 255, 256, 257, 700, 2048}
    assert {c[1] for c in R.FINALIZE} == {4, 176, 1024}
    assert {c[2] for c in R.FINALIZE} >= {3000, R.BIG} and any(c[2] == c[0] for c in R.FINALIZE)
    for P in (257, 700, 2048):
        assert {c[3] for c in R.FINALIZE if c[0] == P} == {"none", "sep", "alias"}
    assert {c[4] for c in R.FINALIZE} == {(True, True), (True, False), (False, True), (False, False)}
    assert {float(c[5]) for c in R.FINALIZE} == {float(R.DECAY), 0.0}
    assert {c[6] for c in R.FINALIZE} == {True, False}
    assert [len(j) for _, j in R.FINALIZE_MULTI] == [1, 2, 3, 4]
    for njobs in R.INFER_MULTI:
        cs = R.infer_multi_jobs(njobs)
        assert len(cs) == njobs
        for i0 in range(0, njobs, 64):          # every launch of two or more jobs mixes a job below its widest with it
            chunk = cs[i0:i0 + 64]
            assert len(chunk) == 1 or min(chunk) + 256 <= max(chunk)
    assert set(R.infer_multi_jobs(130)) == set(R.INFER_C)


# ---- finalize -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.FINALIZE, ids=R.fin_id)
def test_finalize_emulation_passes_every_gate_in_every_contraction(case):
    k = R.build_finalize(*case)
    assert k.stats.shape == (2, k.C, k.P) and k.stats.dtype == F32
    for form in FORMS:
        rep = run_finalize(k, form)
        assert rep["finalize:mean"] <= 1 and rep["finalize:rstd"] <= 1


@pytest.mark.parametrize("jobs", R.FINALIZE_MULTI, ids=lambda j: "%djobs" % len(j[1]))
def test_finalize_multi_jobs_pass_every_gate(jobs):
    decay, js = jobs
    for i, j in enumerate(js):
        k = R.build_finalize(*j, decay=decay, seed=10 + i)
        for form in FORMS:
            run_finalize(k, form)


PLANTS_FIN = [("last partial dropped", lambda k: k.P >= 2),
              ("second stride trip dropped", lambda k: k.P > 256),
              ("unbiased variance", lambda k: k.count > 1),
              ("pivot added twice", lambda k: k.pivot is not None),
              ("mean_c taken for mean", lambda k: k.pivot is not None),
              ("rstd off by 4 ulps", lambda k: True)]


@pytest.mark.parametrize("plant", PLANTS_FIN, ids=lambda p: p[0].replace(" ", "_"))
def test_planted_finalize_defect_fails_a_gate(plant):
    name, has_path = plant
    k = smallest(R.FINALIZE, _fin, has_path)
    run_finalize(k, "mul_add")
    with pytest.raises(AssertionError, match="outside the gate"):
        run_finalize(k, "mul_add", plant=name)
    with pytest.raises(AssertionError, match="outside the gate"):
        run_finalize(k, "fma", plant=name)


# ---- apply ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,z16", [(s, False) for s in R.APPLY] + [(s, True) for s in R.APPLY_Z16],
                         ids=lambda v: R.apply_id(v) if isinstance(v, tuple) else ("z16" if v else "z32"))
def test_apply_emulation_passes_every_gate_in_either_contraction(shape, z16):
    k = R.build_apply(*shape, z16=z16)
    if z16:
        assert np.array_equal(bf16_round(k.z), k.z)
    for form in ("mul_add", "fma"):
        R.check_apply(k, *emulate_apply(k, form))


def test_apply_cases_reach_what_they_claim():
    """Segment layouts: one segment, the 64 | 96 | 16 split with two slices in one wider row, four segments out of channel
    order, mixed storage, records on some segments, all-negative segments with and without a record, bf16 ties in a bf16
    segment whose lower neighbour is odd (where truncation and round-to-even part)."""
    lay = {s: R.build_apply(*s) for s in R.APPLY}
    assert len(lay[(1, 4)].segs) == 1 and len(lay[(140001, 64)].segs) == 1
    k = lay[(777, 176)]
    assert [(s[0], s[1]) for s in k.segs] == [(0, 64), (64, 160), (160, 176)] and k.segs[0][2] == k.segs[2][2]
    assert k.buffers[k.segs[0][2]][0] > 64 + 16
    k = lay[(1, 1024)]
    assert len(k.segs) == 4 and [s[0] for s in k.segs] != sorted(s[0] for s in k.segs)
    assert any(s[0] % 256 for s in k.segs)                                        # a cut inside a wave's 256 channels
    for k in lay.values():
        assert sorted(c for s in k.segs for c in range(s[0], s[1], 4)) == list(range(0, k.C, 4))
        for (c0, c1, bi, col, _, neg) in k.segs:
            assert col % 4 == 0 and col + c1 - c0 <= k.buffers[bi][0] and k.buffers[bi][0] % 4 == 0
            assert (k.hi[:, c0:c1].max() == 0) == neg
    mixed = [k for k in lay.values() if {k.buffers[s[2]][1] for s in k.segs} == {R.DT_F32, R.DT_BF16}]
    some = [k for k in lay.values() if 0 < sum(s[4] for s in k.segs) < len(k.segs)]
    assert len(mixed) >= 4 and len(some) >= 4
    assert any(s[5] and s[4] for k in lay.values() for s in k.segs) and any(s[5] and not s[4] for k in lay.values() for s in k.segs)
    k = lay[(777, 176)]
    c0, c1 = k.segs[1][0], k.segs[1][1]
    assert k.buffers[k.segs[1][2]][1] == R.DT_BF16
    t = k.t[:, c0:c1][:, (np.arange(c0, c1) % 8 == 1)]
    t = t[k.z[:, c0:c1][:, (np.arange(c0, c1) % 8 == 1)] != 0]
    down = (t.astype(F32).view(np.uint32) & np.uint32(0xFFFF0000)).view(F32)
    odd = (down.view(np.uint32) >> 16) & 1
    assert (bf16_round(t.astype(F32)) != down)[odd == 1].all() and (bf16_round(t.astype(F32)) == down)[odd == 0].all()
    assert odd.sum() > 100 and (1 - odd).sum() > 100
    # the kink: values whose z rstd + shift is within an fp32 rounding of 0, of either sign
    kc = np.arange(k.C) % 8 == 3
    at_kink = k.z[:, kc] != 0
    assert (np.abs(k.t[:, kc]) <= 4 * R.ulp32(k.shift[kc].astype(np.float64)))[at_kink].all()
    assert (k.t[:, kc] > 0)[at_kink].any() and (k.t[:, kc] < 0)[at_kink].any()


PLANTS_APPLY = [("column group in the neighbouring segment", lambda k: len(k.segs) >= 2),
                ("stale row in the second pass", lambda k: R.rows_per_thread(k.M, k.C)[0] >= 3),
                ("truncation to bf16", lambda k: any(k.buffers[s[2]][1] == R.DT_BF16 for s in k.segs))]


@pytest.mark.parametrize("plant", PLANTS_APPLY, ids=lambda p: p[0].replace(" ", "_"))
def test_planted_apply_defect_fails_a_gate(plant):
    name, has_path = plant
    k = smallest(R.APPLY, _app, has_path)
    for form in ("mul_add", "fma"):
        with pytest.raises(AssertionError, match="outside the gate"):
            R.check_apply(k, *emulate_apply(k, form, plant=name))


def test_a_record_that_misses_a_segment_or_leaks_into_another_fails():
    k = R.build_apply(7, 12)
    bufs, recs = emulate_apply(k, "fma")
    R.check_apply(k, bufs, recs)
    recs[1][32] = F32(1e6)                      # another segment's maximum in this segment's record
    with pytest.raises(AssertionError, match="record"):
        R.check_apply(k, bufs, recs)
    bufs, recs = emulate_apply(k, "fma")
    recs[1][:] = np.where(np.arange(R.AMAX_FLOATS) % 32 == 0, 0, recs[1])      # the segment's maximum never recorded
    with pytest.raises(AssertionError, match="record"):
        R.check_apply(k, bufs, recs)


# ---- infer prepare ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", R.INFER_C)
def test_infer_emulation_passes_and_a_4_ulp_error_fails(C):
    k = R.build_infer(C)
    assert (k.mv >= 0).all() and (k.mv == 0).any() == (C >= 1)
    for form in ("mul_add", "fma"):
        R.check_infer(k, *emulate_infer(k, form))
        # the documented error of sqrtf is inside the gate ...
        R.check_infer(k, *emulate_infer(k, form, plant="sqrtf faithful, not nearest"))
        # ... four ulps of rstd are not
        with pytest.raises(AssertionError, match="rstd"):
            R.check_infer(k, *emulate_infer(k, form, plant="rstd off by 4 ulps"))
    if C >= 255:
        near = k.mv <= 1e-7
        assert near.any() and (np.abs(k.r_ref[near] - 1 / math.sqrt(float(R.EPS))) < 2e-3).all() and (k.mv >= 3e4).any()


def test_infer_multi_jobs_pass():
    for j, C in enumerate(R.infer_multi_jobs(130)):
        k = R.build_infer(C, seed=j)
        R.check_infer(k, *emulate_infer(k, "mul_add" if j % 2 else "fma"))


# ---- argument checks that answer without a device ---------------------------------------------------------------------------------------
def test_five_finalize_jobs_are_refused_with_a_message():
    from tumblr_emotions_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(ROOT, "tumblr_emotions_amd", "csrc"), "-j4"], check=True)
    lib = _lib.load()
    jobs = (_lib.BnFinalizeJob * 5)()
    assert lib.ds_bn_finalize_multi(ctypes.cast(jobs, ctypes.c_void_p), 5, float(R.EPS), float(R.DECAY), None) == -1
    assert b"ds_bn_finalize_multi: 1..4 jobs required" in lib.ds_last_error()
    assert lib.ds_bn_finalize_multi(ctypes.cast(jobs, ctypes.c_void_p), 0, float(R.EPS), float(R.DECAY), None) == -1
    # a job without its vectors is refused before anything is launched
    assert lib.ds_bn_finalize_multi(ctypes.cast(jobs, ctypes.c_void_p), 4, float(R.EPS), float(R.DECAY), None) == -1
    assert b"job 0 is malformed" in lib.ds_last_error()
    assert lib.ds_bn_infer_prepare_multi(ctypes.cast((_lib.BnInferJob * 1)(), ctypes.c_void_p), 0, float(R.EPS), None) == -1
