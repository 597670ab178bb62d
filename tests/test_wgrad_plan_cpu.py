"""The host decision of ds_conv_wgrad -- which kernel, which tile shape, how many split-K slabs, which vector widths -- read
back through ds_debug_conv_wgrad_plan of the tuning library over the case table of wgrad_cases.py and every pointer and
leading-dimension alignment.  No device needed: the query launches nothing, and ds_conv_wgrad refuses a short workspace
before it launches anything."""
import ctypes as C
import itertools

import pytest

import wgrad_cases as K

BASE = 0x7f0000001000                  # a 256-byte aligned address that is never dereferenced
DS_ERR_ARG, DS_ERR_WORKSPACE = -1, -3


@pytest.fixture(scope="module")
def lib():
    from tumblr_emotions_amd import _lib
    t = _lib.load_tuning()
    assert t.ds_debug_conv_wgrad_force(0, 0, 0) == 0
    return t


def _plan_at(lib, case, off):
    ptrs = [BASE + o for o in off]
    return K.read_plan(lib, case, *ptrs), case.widths(*ptrs)


def _check(case, plan, widths, ws_bytes, pinned_slabs=0):
    direct, ai, bj, slabs, wx, wz = plan
    assert direct == int(case.M >= 512 and not case.fold), (case, plan)
    assert (wx, wz) == widths, (case, plan, widths)
    if direct:
        assert (ai, bj) in K.TILES and ai <= wx and bj <= wz, (case, plan)
        assert slabs in K.SLABS, (case, plan)
        if pinned_slabs:
            assert slabs == pinned_slabs, (case, plan)
        else:
            assert slabs == 1 or case.M // slabs >= 256, (case, plan)
            assert ws_bytes >= case.ws_need(slabs), (case, plan, ws_bytes)
    else:
        assert (ai, bj) == (0, 0) and slabs >= 1, (case, plan)
        assert ws_bytes >= case.ws_need(slabs), (case, plan, ws_bytes)


def test_plan_invariants_at_every_alignment_of_pointers_and_leading_dimensions(lib):
    """slabs in the allowed set and >= 256 pixels each; ai <= wx, bj <= wz with the widths the rule of max_width gives;
    direct == (M >= 512 and not folded); the workspace of ds_conv_wgrad_workspace -- which does not see the pointers --
    suffices for the slab count of every alignment."""
    shapes = {(c.N, c.H, c.W, c.Cin, c.Cout, c.k, c.stride, c.fold): c for c in K.all_cases()}
    offsets = list(itertools.product((0, 4, 8), repeat=4))
    seen = set()
    for c in shapes.values():
        for ex, ez in itertools.product((0, 1, 2, 4), repeat=2):
            if c.fold and ex:
                continue                      # the folded layout has ldx == fold_cin
            v = c.but(ldx=c.ldx + ex, lddz=c.lddz + ez, off=(0, 0, 0, 0), pin=(0, 0, 0))
            ws_bytes = v.wplan().ws_bytes
            for off in offsets:
                plan, widths = _plan_at(lib, v, off)
                _check(v, plan, widths, ws_bytes)
                seen.add(plan[4:])
    assert seen == set(itertools.product((1, 2, 4), repeat=2))


def test_a_pin_holds_where_the_alignment_allows_it_and_is_ignored_where_not(lib):
    shape = K.PIN_SHAPES[0]
    free = K.read_plan(lib, shape, BASE, BASE, BASE, BASE)
    for (a, b), s in itertools.product(K.TILES, K.PIN_SLABS):
        with K.pinned(lib, (a, b, s)):
            for off in ((0, 0, 0, 0), (8, 0, 0, 0), (4, 0, 0, 0), (0, 8, 0, 0), (0, 0, 4, 0), (0, 0, 0, 8), (4, 4, 4, 4)):
                plan, (wx, wz) = _plan_at(lib, shape, off)
                _check(shape, plan, (wx, wz), 0, pinned_slabs=s)
                # a tile width the operands do not allow is left to the model (which stays within the widths)
                assert plan[1] == (a if a <= wx else plan[1]) and plan[2] == (b if b <= wz else plan[2]), (a, b, s, off, plan)
                if a <= wx and b <= wz:
                    assert plan[:4] == (1, a, b, s)
    assert K.read_plan(lib, shape, BASE, BASE, BASE, BASE) == free
    with K.pinned(lib, (0, 0, 8)):           # a slab count alone: the model's tile
        assert K.read_plan(lib, shape, BASE, BASE, BASE, BASE)[:4] == free[:3] + (8,)
    # the LDS kernel takes no pin
    lds = K.LDS_CASES[0]
    with K.pinned(lib, (2, 2, 4)):
        assert K.read_plan(lib, lds, BASE, BASE, BASE, BASE) == (0, 0, 0, 2, 4, 4)


def test_the_setter_refuses_what_is_no_tile_shape_or_slab_count(lib):
    for bad in ((3, 0, 0), (0, 8, 0), (-1, 0, 0), (0, 0, 3), (0, 0, 12), (0, 0, 72), (0, 0, -8)):
        assert lib.ds_debug_conv_wgrad_force(*bad) == DS_ERR_ARG, bad
        assert b"ds_debug_conv_wgrad_force" in lib.ds_last_error()
    shape = K.PIN_SHAPES[0]
    free = K.read_plan(lib, shape, BASE, BASE, BASE, BASE)
    assert lib.ds_debug_conv_wgrad_force(4, 4, 24) == 0
    assert lib.ds_debug_conv_wgrad_force(5, 4, 24) == DS_ERR_ARG          # a refused call changes nothing
    assert K.read_plan(lib, shape, BASE, BASE, BASE, BASE)[:4] == (1, 4, 4, 24)
    assert lib.ds_debug_conv_wgrad_force(0, 0, 0) == 0
    assert K.read_plan(lib, shape, BASE, BASE, BASE, BASE) == free
    assert lib.ds_debug_conv_wgrad_plan(None, None, None, 0, None, None, (C.c_int * 6)()) == DS_ERR_ARG


def test_the_cases_reach_every_launch_form(lib):
    """What test_wgrad_gpu.py runs: all nine tile shapes ((4,2) and (4,4), which the model never picks, by pinning only), every
    slab count Mixed_5c's four launches take at batches 32 and 256, both ci tiles of the LDS kernel, an empty trailing slab by
    the model's choice, all three widths on either side -- and the plans stated in the table are the library's."""
    tiles, free_tiles, slabs = set(), set(), set()
    for c in K.all_cases():
        with K.pinned(lib, c.pin):
            plan, widths = _plan_at(lib, c, c.off)
        _check(c, plan, widths, max(c.wplan().ws_bytes, c.ws_need(c.pin[2] or 1)), pinned_slabs=c.pin[2] if c.direct else 0)
        if plan[0]:
            tiles.add(plan[1:3])
            slabs.add(plan[3])
            if not any(c.pin):
                free_tiles.add(plan[1:3])
        if c.plan is not None:
            assert plan[:4] == c.plan, (c, plan)
    assert tiles == set(K.TILES)
    assert free_tiles == set(K.TILES) - {(4, 2), (4, 4)}
    for c in K.PIN_CASES:
        with K.pinned(lib, c.pin):
            assert K.read_plan(lib, c, BASE, BASE, BASE, BASE)[:4] == (1,) + c.pin, c
    # Mixed_5c as the step runs it; the batch-256 rows of the table are the smallest batches with the same plan
    for ci, co, k in K.MIXED_5C_LAYERS:
        for B in K.MIXED_5C_BATCHES:
            full = K.read_plan(lib, K.Case(B, 7, 7, ci, co, k, 1), BASE, BASE, BASE, BASE)
            assert full[3] in slabs, (ci, co, k, B, full)
            rows = [c for c in K.MODEL_CASES if (c.H, c.Cin, c.Cout, c.k) == (7, ci, co, k) and c.plan == full[:4]]
            assert rows, (ci, co, k, B, full)
            if B == 256:
                assert full[1:3] == (1, 4)
                n = min(c.N for c in rows)
                assert K.read_plan(lib, K.Case(n - 1, 7, 7, ci, co, k, 1), BASE, BASE, BASE, BASE) != full
    assert {K.lds_ci_tile(c.Cin) for c in K.LDS_CASES} == {64, 128}
    assert any(c.fold and c.M >= 512 for c in K.LDS_CASES) and any(c.fold and c.M < 512 for c in K.LDS_CASES)
    e = K.EMPTY_SLAB_CASE
    pix = -(-(-(-e.M // 64)) // 8) * 8          # pixels per slab: ceil(M / slabs) rounded up to 8
    assert K.read_plan(lib, e, BASE, BASE, BASE, BASE)[3] == 64 and 63 * pix >= e.M > 62 * pix
    assert {K.read_plan(lib, c, *(BASE + o for o in c.off))[4] for c in K.LAYOUT_CASES} == {1, 2, 4}
    assert {K.read_plan(lib, c, *(BASE + o for o in c.off))[5] for c in K.LAYOUT_CASES} == {1, 2, 4}
    for c, ctl in zip(K.DEAD_TAP_CASES, K.DEAD_TAP_CONTROLS):
        assert K.dead_taps(c) and K.dead_taps(c) == K.dead_taps(ctl) and c.direct and not ctl.direct
    assert not any(K.dead_taps(c) for c in K.DOUBLE_WRAP_CASES + K.PIN_SHAPES)


@pytest.mark.parametrize("which", ["product", "tuning"])
def test_a_workspace_one_byte_short_is_refused_before_any_launch(lib, which):
    from tumblr_emotions_amd import _lib
    L = _lib.load() if which == "product" else lib
    for case in (K.MODEL_CASES[0], K.LDS_CASES[0]):
        plan = case.wplan()
        slabs = K.read_plan(lib, case, BASE, BASE, BASE, BASE)[3]
        need = case.ws_need(slabs)
        assert slabs > 1 and plan.ws_bytes >= need > 0
        p = C.c_void_p(BASE)
        for ws, nbytes in ((p, need - 1), (p, 0), (None, need)):
            rc = L.ds_conv_wgrad(C.byref(plan.d), p, p, case.lddz, p, ws, nbytes, None)
            assert rc == DS_ERR_WORKSPACE, (case, nbytes)
            assert b"ds_conv_wgrad: workspace" in L.ds_last_error() and str(need).encode() in L.ds_last_error()
