"""wide_cases.py without a device: the builders' exactness assertions over the whole table, the comparison helpers against
planted errors, and the host launch choice (ds_debug_conv_igemm_launch of the tuning library) over the table x pinned NB --
all 34 instantiations of gemm_wide_kernel that kernel_of() names, and nothing else."""
import ctypes as C

import numpy as np
import pytest

import wide_cases as W

# (NB, n-contiguous weights, BNB, POOL, BNR): gemm_wide_kernel<NB, BNMAJOR, BNB, POOL, BNR> as kernel_of() names them
THE_34 = {
    (1, 1, 0, 0, 0), (2, 1, 0, 0, 0), (3, 1, 0, 0, 0), (4, 1, 0, 0, 0), (5, 1, 0, 0, 0), (6, 1, 0, 0, 0), (7, 1, 0, 0, 0), (8, 1, 0, 0, 0),
    (1, 0, 0, 0, 0), (2, 0, 0, 0, 0), (3, 0, 0, 0, 0), (4, 0, 0, 0, 0), (5, 0, 0, 0, 0), (6, 0, 0, 0, 0), (7, 0, 0, 0, 0), (8, 0, 0, 0, 0),
    (1, 0, 1, 0, 0), (2, 0, 1, 0, 0),
    (1, 1, 0, 1, 0), (2, 1, 0, 1, 0), (3, 1, 0, 1, 0), (4, 1, 0, 1, 0),
    (1, 1, 0, 0, 1), (2, 1, 0, 0, 1), (3, 1, 0, 0, 1), (4, 1, 0, 0, 1), (5, 1, 0, 0, 1), (6, 1, 0, 0, 1), (7, 1, 0, 0, 1), (8, 1, 0, 0, 1),
    (1, 1, 0, 1, 1), (2, 1, 0, 1, 1), (3, 1, 0, 1, 1), (4, 1, 0, 1, 1),
}


@pytest.fixture(scope="module")
def lib():
    from tumblr_emotions_amd import _lib
    return _lib.load_tuning()


def test_the_builders_exactness_assertions_hold_for_the_whole_table():
    """build() asserts the quantum / 2^24 condition for z and for every statistics partial; here also what each builder
    promises about its operands."""
    assert len(THE_34) == 34 and W.ALL_INSTANTIATIONS == THE_34
    seen_modes = set()
    for c in W.all_cases():
        p = W.build(c)
        seen_modes.add((c.variant, c.mode))
        K, N = c.K, c.Cout
        assert p.x.shape == (c.M, K + 8) and (p.x[:, K:] == W.X_PAD).all()
        assert W.is_multiple(p.w, 1.0) and np.abs(p.w).max() <= (1 if K >= 1024 else 2)
        if not c.bnb:
            assert W.is_multiple(p.x[:, :K], 1.0)
        if c.norm:
            r, s = p.rstd.astype(np.float64), p.shift.astype(np.float64)
            assert set(np.unique(r)) <= {0.5, 1.0, 2.0} and W.is_multiple(s, 0.25)
            q = K // 4
            assert (r[:q] == 1).all() and (s[:q] == 0).all() and (p.x[:, :q] >= 0).all()
            t = p.x[:, q:K] * r[q:] + s[q:]
            assert ((t < 0).any(0) & (t == 0).any(0) & (t > 0).any(0)).all()
        if c.bnb:
            assert c.ends[-1] == K and all(e % 16 == 0 for e in c.ends[:-1]) and len(p.dy_parts) == len(c.ends)
            assert len({part.shape[1] for _, _, part in p.dy_parts}) == len(p.dy_parts)          # their own strides
            assert all(part.shape[1] > c1 - c0 and part.shape[1] % 4 == 0 for c0, c1, part in p.dy_parts)
        if c.mode == "stats":
            assert W.is_multiple(p.pivot, 1.0) and (p.pivot != 0).all()
        if c.mode == "stats0":
            assert p.pivot is None
        if c.flags & W.EPI_BNSUMS:
            zeros = (p.y == 0).mean()
            assert W.is_multiple(p.y, 0.25) and 0.15 < zeros < 0.6, zeros
            assert p.mask.shape[1] > N and (p.mask[:, N:] > 0).all()
            if c.mode.endswith("_rstd"):
                assert (p.mask_shift > 0).any()          # rows past M (read as 0) must not switch on
        if c.bnr:
            assert (p.z[:, N // 2] == 0).all() and W.is_multiple(p.scale, 0.5) and W.is_multiple(p.bn_shift, 0.25)
        if c.pool:
            assert p.winners.shape == (c.M, K) and p.winners.max() <= 8
    assert seen_modes == {(v, m) for v in W.VARIANTS for m in W.VARIANTS[v][2]}
    # the table names the geometry it promises
    for nb in range(1, 9):
        ms, ks, ns = (set(s[i] for s in W.shapes(nb)) for i in range(3))
        assert ms == {165, 37, 256} and ks >= {32, 40, 296} and ns == {32 * nb - 28, 32 * nb + 4}
        assert (1024 in ks) == (nb in (2, 8))
    assert {len(e) for e in W.BNB_ENDS.values()} == {1, 2, 3} and W.BNB_ENDS[40] == (16, 32, 40)
    assert {co for v in W.POOL_COUT.values() for co in v} == {32, 40, 96, 100, 128}
    assert {m[:3] for m in W.POOL_MAPS} == {(3, 14, 14), (5, 7, 7), (2, 28, 28), (3, 9, 11)}


def _first(variant, nb, mode, **kw):
    return next(c for c in W.cases(variant, nb) if c.mode == mode and all(getattr(c, k) == v for k, v in kw.items()))


def test_the_comparison_helpers_reject_planted_errors():
    c = _first("fwd", 3, "stats", M=165, Cout=100)
    p = W.build(c)
    good = W.z_buffer(p)
    good[W.GUARD_ROWS:W.GUARD_ROWS + c.M, :c.Cout] = p.z
    W.check_z(good, p)
    sgood = W.stats_buffer(p)
    sgood[:2 * c.Cout * c.partials] = p.stats.reshape(-1)
    W.check_stats(sgood, p)
    # one element off by one quantum
    bad = good.copy()
    bad[W.GUARD_ROWS + 164, 99] += p.quantum
    with pytest.raises(AssertionError, match="z differs at 1 of"):
        W.check_z(bad, p)
    # one canary overwritten: a column right of Cout, a guard row in front, a guard row behind
    for pos in ((W.GUARD_ROWS + 5, c.Cout), (W.GUARD_ROWS - 1, 0), (W.GUARD_ROWS + c.M, 3)):
        bad = good.copy()
        bad[pos] = 0.0
        with pytest.raises(AssertionError, match="guard"):
            W.check_z(bad, p)
    # one row dropped from one partial; a phantom row of -pivot (its square in the second sum)
    pv = p.pivot.astype(np.float64)
    st = p.stats.copy()
    st[0, :, 1] -= p.z[164] - pv
    st[1, :, 1] -= (p.z[164] - pv) ** 2
    bad = sgood.copy()
    bad[:st.size] = st.reshape(-1)
    with pytest.raises(AssertionError, match="statistics differ"):
        W.check_stats(bad, p)
    st = p.stats.copy()
    st[0, :, 1] += -pv
    st[1, :, 1] += pv ** 2
    bad = sgood.copy()
    bad[:st.size] = st.reshape(-1)
    with pytest.raises(AssertionError, match="statistics differ"):
        W.check_stats(bad, p)
    bad = sgood.copy()
    bad[7] = np.nan
    with pytest.raises(AssertionError, match="not written"):
        W.check_stats(bad, p)
    bad = sgood.copy()
    bad[-1] = 0.0
    with pytest.raises(AssertionError, match="canary"):
        W.check_stats(bad, p)
    # the sums of the right total in the wrong partial are refused for a launch that is not pooled
    st = p.stats.copy()
    st[0, 0, 0], st[0, 0, 1] = st[0, 0, 0] + 1, st[0, 0, 1] - 1
    bad = sgood.copy()
    bad[:st.size] = st.reshape(-1)
    with pytest.raises(AssertionError, match="statistics differ"):
        W.check_stats(bad, p)
    # one winner byte changed, one left unwritten, the canary behind
    c = _first("pool", 2, "stats", hw=(5, 7, 7))
    p = W.build(c)
    wgood = W.winners_buffer(p)
    wgood[:c.M * c.K] = p.winners.reshape(-1)
    W.check_winners(wgood, p)
    bad = wgood.copy()
    bad[11] = (bad[11] + 1) % 9
    with pytest.raises(AssertionError, match="winners differ at 1 of"):
        W.check_winners(bad, p)
    bad = wgood.copy()
    bad[11] = W.WINNER_FILL
    with pytest.raises(AssertionError, match="not written"):
        W.check_winners(bad, p)
    bad = wgood.copy()
    bad[c.M * c.K] = 0
    with pytest.raises(AssertionError, match="canary"):
        W.check_winners(bad, p)
    # the real-valued gate: a partial off by more than its bound
    rc = W.real_case("fwd", 3)
    rp = W.build(rc)
    z32 = rp.z.astype(np.float32)
    sb = W.stats_buffer(rp)
    pv = rp.pivot.astype(np.float64)
    z64 = z32.astype(np.float64)
    for i in range(rc.partials):
        rows = slice(128 * i, min(rc.M, 128 * i + 128))
        sb[:2 * rc.Cout * rc.partials].reshape(2, rc.Cout, rc.partials)[0, :, i] = (z64[rows] - pv).sum(0)
        sb[:2 * rc.Cout * rc.partials].reshape(2, rc.Cout, rc.partials)[1, :, i] = ((z64[rows] - pv) ** 2).sum(0)
    assert W.real_stats_check(sb, rp, z32) < 0.1          # (the cast of an fp64 sum to fp32: one unit of 132)
    sb[1] += -pv[0]
    with pytest.raises(AssertionError, match="off by"):
        W.real_stats_check(sb, rp, z32)


def _query_desc(lib, c, keep):
    """The case's descriptor as the launch gets it (the on-load pointers are only looked at for being set)."""
    from tumblr_emotions_amd import _lib
    d = W.make_desc(c)
    if c.bnb:
        b = _lib.BnBwdOnLoad()
        keep.append(b)
        d.bnb = C.addressof(b)
    if c.pool:
        buf = C.create_string_buffer(16)
        keep.append(buf)
        d.pool_argmax = C.addressof(buf)
    return d


def test_the_table_under_its_pins_reaches_all_34_instantiations_and_nothing_else(lib):
    reached, keep = set(), []
    try:
        for c in W.all_cases() + [W.real_case(v, nb) for v, nb in W.VARIANT_NB]:
            with W.pinned(lib, c.nb):
                got = W.launch_of(lib, _query_desc(lib, c, keep))
            inst, wgs, partials = W.expected_launch(c)
            assert got[:5] == inst, (c, got)
            assert got[6] == c.nb and got[7] == 0 and got[8] == wgs and got[9] == partials, (c, got)
            reached.add(got[:5])
        assert reached == THE_34, sorted(reached ^ THE_34)
        # every non-pooled pin is reached with one column tile AND with two
        for v, nb in W.VARIANT_NB:
            if v not in ("pool", "poolnorm", "poolbnr"):
                assert {c.col_tiles for c in W.cases(v, nb)} == {1, 2}
    finally:
        lib.ds_debug_conv_set_wide(1)
        lib.ds_debug_conv_set_wide_nb(0)


def test_the_pin_is_checked_and_a_launchs_own_cap_holds(lib):
    try:
        assert lib.ds_debug_conv_set_wide_nb(9) == -1 and b"ds_debug_conv_set_wide_nb" in lib.ds_last_error()
        assert lib.ds_debug_conv_set_wide_nb(-1) == -1
        keep = []
        c = next(c for c in W.cases("bnb", 2) if c.Cout == 68 and c.mode == "plain")
        plain = next(k for k in W.cases("dgrad", 2) if (k.M, k.K, k.Cout, k.mode) == (c.M, c.K, c.Cout, "plain"))
        pool = next(k for k in W.cases("pool", 4) if k.Cout == 100)
        with W.pinned(lib, 5):
            assert W.launch_of(lib, W.make_desc(plain))[0] == 5
            got = W.launch_of(lib, _query_desc(lib, c, keep))
            assert 1 <= got[0] <= 2 and got[2] == 1, got          # a pin above the cap of two is ignored
            assert W.launch_of(lib, _query_desc(lib, pool, keep))[0] == 4          # POOL keeps ceil(Cout / 32)
        with W.pinned(lib, 1):
            assert W.launch_of(lib, _query_desc(lib, pool, keep))[0] == 4
        # 0 = the cost model: what the launch is without the new switch
        with W.pinned(lib, 0):
            free = W.launch_of(lib, W.make_desc(plain))
        assert lib.ds_debug_conv_set_wide(2) == 0
        assert W.launch_of(lib, W.make_desc(plain)) == free and free[0] in (2, 3)
        assert lib.ds_debug_conv_igemm_launch(None, None) == -1
    finally:
        lib.ds_debug_conv_set_wide(1)
        lib.ds_debug_conv_set_wide_nb(0)
    # the defaults: a small shape stays on the LDS-tile kernels (too few workgroups for the wide kernel)
    got = W.launch_of(lib, W.make_desc(plain))
    assert got[0] == 0 and got[5] >= 1 and got[6] >= 1
