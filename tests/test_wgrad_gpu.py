"""ds_conv_wgrad against S.conv2d_same_bwd_filter in fp64: every instantiation of the register-direct kernel at every slab
form, the cycle model's own choices, every operand layout, the LDS kernel's forms, and geometries with taps that never touch
the image (wgrad_cases.py has the table; test_wgrad_plan_cpu.py checks without a device what the table reaches).

The main operands are integers of {-3 .. 3} stored as fp32: every product and every partial sum is an integer of magnitude
<= 9 M < 2^24, so the fp32 MFMA chain, the sum of the four waves through LDS and splitk_reduce_kernel are exact in any order
and dw must EQUAL the oracle.  Small integers are exact in bf16 too, so every case also runs standard-normal operands at the
bound of test_conv_wgrad, 3e-4 of max|ref|.  x and dz lie in NaN: the columns between Cin and ldx (Cout and lddz), and the
floats before and after the tensors -- whatever is read outside the operands poisons dw.  dw starts as NaN between canaries;
the workspace starts as NaN (a slab that is never written poisons dw) with a canary behind the bytes the call is given."""
import ctypes as C
import zlib

import numpy as np
import pytest
import torch

import wgrad_cases as K

pytestmark = pytest.mark.gpu

GUARD = 64                  # floats on either side of a tensor (256 bytes: the tensor keeps the allocation's alignment)
CANARY = 12345.0
_DATA = {}


def data(case, gaussian=False):
    """(x, dz, ref) of the case's geometry, computed once per module and never written."""
    key = (case.N, case.H, case.W, case.Cin, case.Cout, case.k, case.stride, case.fold, gaussian)
    if key not in _DATA:
        x, dz = K.operands(case, zlib.crc32(repr(key).encode()), gaussian)
        ref = K.reference(case, x, dz)
        if not gaussian:
            assert 9 * case.M < 2 ** 24 and np.array_equal(ref, np.rint(ref)) and np.abs(ref).max() < 2 ** 24
        for a in (x, dz, ref):
            a.setflags(write=False)
        _DATA[key] = (x, dz, ref)
    return _DATA[key]


def _rows_in_nan(rows, ld, off):
    """rows [R, C] as R rows of ld floats at byte offset off behind GUARD floats of NaN, NaN everywhere else."""
    R, Cc = rows.shape
    host = np.full(GUARD + off // 4 + R * ld + GUARD, np.nan, np.float32)
    host[GUARD + off // 4:GUARD + off // 4 + R * ld].reshape(R, ld)[:, :Cc] = rows
    return torch.from_numpy(host).cuda()


class Launch:
    """The four device buffers of a case and one call of ds_conv_wgrad on them."""

    def __init__(self, case, x, dz):
        self.case = c = case
        self.x = _rows_in_nan(x.reshape(-1, x.shape[-1]), c.ldx, c.off[0])
        self.dz = _rows_in_nan(dz.reshape(-1, c.Cout), c.lddz, c.off[1])
        self.plan = c.wplan()
        self.ws_bytes = max(self.plan.ws_bytes, c.ws_need(max(K.PIN_SLABS)))
        self.dw = torch.empty(GUARD + c.off[2] // 4 + c.n_dw + GUARD, device="cuda")
        self.ws = torch.empty(c.off[3] // 4 + self.ws_bytes // 4 + GUARD, device="cuda")
        for t in (self.x, self.dz, self.dw, self.ws):
            assert t.data_ptr() % 256 == 0
        self.ptrs = (self.x.data_ptr() + 4 * GUARD + c.off[0], self.dz.data_ptr() + 4 * GUARD + c.off[1],
                     self.dw.data_ptr() + 4 * GUARD + c.off[2], self.ws.data_ptr() + c.off[3])

    def read_plan(self, lib):
        return K.read_plan(lib, self.case, *self.ptrs)

    def run(self, ws_bytes):
        """dw [KH, KW, Cin, Cout] (fp64 on the host) of one call given ws_bytes of workspace; the canaries are checked."""
        c = self.case
        assert ws_bytes <= self.ws_bytes
        lo, n = GUARD + c.off[2] // 4, c.n_dw
        self.dw.fill_(CANARY)
        self.dw[lo:lo + n] = float("nan")
        self.ws.fill_(float("nan"))
        self.ws[(c.off[3] + ws_bytes) // 4:] = CANARY
        x, dz, dw, ws = (C.c_void_p(p) for p in self.ptrs)
        self.plan.run(x, dz, dw, ws, ws_bytes)
        torch.cuda.synchronize()
        got = self.dw.cpu().numpy()
        assert (got[:lo] == CANARY).all() and (got[lo + n:] == CANARY).all(), "%s: written outside dw" % c
        assert (self.ws[(c.off[3] + ws_bytes) // 4:] == CANARY).all().item(), "%s: written behind the workspace" % c
        return got[lo:lo + n].astype(np.float64).reshape(c.KH, c.KW, c.Cin, c.Cout)


def gaussian_error(lib, case, pin=(0, 0, 0)):
    """max |dw - ref| / max |ref| of the case with standard-normal operands (asserted at 3e-4, test_conv_wgrad's bound)."""
    x, dz, ref = data(case, gaussian=True)
    L = Launch(case, x, dz)
    with K.pinned(lib, pin):
        slabs = L.read_plan(lib)[3]
        dw = L.run(max(L.plan.ws_bytes, case.ws_need(slabs)) if any(pin) else L.plan.ws_bytes)
    assert np.isfinite(dw).all(), case
    err = np.abs(dw - ref).max() / max(1e-6, np.abs(ref).max())
    print("WGRAD gaussian %s pin %s: %.3e" % (case, pin, err))
    assert err <= 3e-4, (case, pin, err)
    return err


def exact(lib, case, pin=None, want_plan=None):
    """One call with the integer operands: the read-back plan obeys the rules (and equals want_plan), the workspace the case
    is entitled to suffices, dw equals the oracle.  Returns (dw, plan)."""
    pin = case.pin if pin is None else pin
    x, dz, ref = data(case)
    L = Launch(case, x, dz)
    with K.pinned(lib, pin):
        plan = L.read_plan(lib)
        direct, ai, bj, slabs, wx, wz = plan
        assert direct == int(case.direct) and (wx, wz) == case.widths(*L.ptrs), (case, plan)
        if direct:
            assert ai <= wx and bj <= wz and slabs in K.SLABS, (case, plan)
        if want_plan is not None:
            assert plan[:4] == tuple(want_plan), (case, plan, want_plan)
        # a pinned plan's workspace is the caller's to size (a pinned tile takes the slab count the model gives that tile);
        # otherwise ds_conv_wgrad_workspace must do
        ws_bytes = max(L.plan.ws_bytes, case.ws_need(slabs)) if any(pin) else L.plan.ws_bytes
        assert ws_bytes >= case.ws_need(slabs), (case, plan, ws_bytes)
        dw = L.run(ws_bytes)
    print("WGRAD plan %s pin %s: %s" % (case, pin, plan))
    bad = np.argwhere(dw != ref)
    assert np.array_equal(dw, ref), "%s plan %s: %d of %d entries differ, first (tap row, tap column, ci, co) %s, taps %s" % (
        case, plan, len(bad), ref.size, bad[0].tolist(), sorted({(int(a), int(b)) for a, b in bad[:, :2]}))
    return dw, plan


@pytest.mark.parametrize("shape", K.PIN_SHAPES, ids=repr)
def test_every_instantiation_at_every_slab_form(shape, tuning_lib):
    """All nine wgrad_direct_kernel<AI, BJ> x slabs in {1, 2, 4, 8, 24} (at 24 the last slab is empty): the plan read back is the
    plan pinned, dw equals the oracle -- hence is equal across tiles and slab counts -- and two runs give the same bits."""
    x, dz, ref = data(shape)
    L = Launch(shape, x, dz)
    worst = 0.0
    for c in K.PIN_CASES:
        if (c.N, c.H, c.stride) != (shape.N, shape.H, shape.stride):
            continue
        dw, plan = exact(tuning_lib, c, want_plan=(1,) + c.pin)
        with K.pinned(tuning_lib, c.pin):
            assert L.read_plan(tuning_lib)[:4] == (1,) + c.pin
            again = L.run(c.ws_need(c.pin[2]))
        assert np.array_equal(again.view(np.uint64), dw.view(np.uint64)), c
        worst = max(worst, gaussian_error(tuning_lib, shape, c.pin))
    print("WGRAD gaussian worst of %s over the pins: %.3e" % (shape, worst))


@pytest.mark.parametrize("case", K.MODEL_CASES, ids=repr)
def test_the_models_own_choices(case, tuning_lib):
    """Nothing pinned: one shape per tile shape the cycle model picks, Mixed_5c's launches with the plans of batches 32 and 256,
    and M = 511 against 512 (the LDS kernel against the direct one).  The plan is the one the table states."""
    exact(tuning_lib, case, want_plan=case.plan)
    gaussian_error(tuning_lib, case)


def test_an_empty_trailing_slab_chosen_by_the_model(tuning_lib):
    """M = 16400: 64 slabs of 264 pixels, slab 63 starts behind M and must still be written (as zeros)."""
    c = K.EMPTY_SLAB_CASE
    _, plan = exact(tuning_lib, c, want_plan=c.plan)
    assert plan[3] == 64
    gaussian_error(tuning_lib, c)


@pytest.mark.parametrize("case", K.LAYOUT_CASES, ids=repr)
def test_operand_layouts_of_the_direct_kernel(case, tuning_lib):
    """x, dz, dw or ws 4 or 8 bytes off a 16-byte boundary, ldx > Cin, lddz > Cout: the widths read back are the rule's, and the
    result is exact with the model's tile, with the widest tile the widths allow, and with (4, 4) pinned (which the call takes
    only as far as the widths allow)."""
    _, plan = exact(tuning_lib, case)
    wx, wz = plan[4:]
    _, widest = exact(tuning_lib, case, pin=(wx, wz, case.pin[2]))
    assert widest[1:3] == (wx, wz)
    _, p44 = exact(tuning_lib, case, pin=(4, 4, case.pin[2]))
    assert p44[1] <= wx and p44[2] <= wz and (p44[1] == 4) == (wx == 4) and (p44[2] == 4) == (wz == 4)
    if case.pin[2]:
        assert plan[3] == widest[3] == p44[3] == case.pin[2]
    gaussian_error(tuning_lib, case, pin=(wx, wz, case.pin[2]))


@pytest.mark.parametrize("case", K.LDS_CASES, ids=repr)
def test_the_lds_kernel(case, tuning_lib):
    """M < 512: stride 2 with odd extents, 16-byte and scalar loads of either operand, both ci tiles, and the folded stem layout
    (which stays on this kernel at M >= 512 too) against the 7 x 7 x 4 filter gradient of the image."""
    _, plan = exact(tuning_lib, case)
    assert plan[:3] == (0, 0, 0) and plan[3] > 1
    gaussian_error(tuning_lib, case)


@pytest.mark.parametrize("case", K.DEAD_TAP_CASES + K.DEAD_TAP_CONTROLS, ids=repr)
def test_taps_that_never_touch_the_image(case, tuning_lib):
    """A 3-tap filter over an extent of 1, the far taps of a stride-2 filter wider than the image: such a tap's x is padding at
    every pixel and its dw is zero -- on the direct kernel, whose padding test is a range compare per axis, as on the LDS
    kernel (the same geometry below 512 pixels)."""
    dw, plan = exact(tuning_lib, case)
    dead = K.dead_taps(case)
    assert dead and all((dw[a, b] == 0).all() for a, b in dead)
    gaussian_error(tuning_lib, case)


@pytest.mark.parametrize("case", K.DOUBLE_WRAP_CASES, ids=repr)
def test_two_row_wraps_per_step_without_dead_taps(case, tuning_lib):
    """OW == 1 with OH > 1: the pixel walk of the direct kernel wraps a row twice per step."""
    _, plan = exact(tuning_lib, case)
    assert plan[0] == 1
    gaussian_error(tuning_lib, case)
