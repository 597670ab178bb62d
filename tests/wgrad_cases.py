"""The launch forms of ds_conv_wgrad, shared by test_wgrad_plan_cpu.py (the host decision, read back through
ds_debug_conv_wgrad_plan without a device) and test_wgrad_gpu.py (the kernels against the fp64 oracle).  A case is one call:
a geometry, the leading dimensions and byte offsets of its four buffers, a pinned (ai, bj, slabs) or none, and -- where the
cycle model's own choice is the point of the case -- the plan the library must report for it."""
import ctypes as C

import numpy as np

from tumblr_emotions_amd import ops

SLABS = (1, 2, 4, 8, 16, 24, 32, 40, 48, 56, 64)              # split-K slab counts of the direct kernel
TILES = tuple((a, b) for a in (1, 2, 4) for b in (1, 2, 4))    # wgrad_direct_kernel<AI, BJ>
PIN_SLABS = (1, 2, 4, 8, 24)
DIRECT_MIN_M = 512


class Case:
    """(N, H, W, Cin, Cout, k, stride) as in WGRAD_DIRECT_CASES; ldx / lddz default to the channel counts; off = byte offsets of
    (x, dz, dw, ws) from a 256-byte aligned address; pin = (ai, bj, slabs) for ds_debug_conv_wgrad_force; fold: the stem layout
    (KW folded into the channel axis: Cin = 7 * 4, ldx = 4, KH = 7, KW = 1); plan = (direct, ai, bj, slabs) the library reports
    for aligned operands with nothing pinned (None: not stated)."""

    def __init__(self, N, H, W, Cin, Cout, k, stride, ldx=None, lddz=None, off=(0, 0, 0, 0), pin=(0, 0, 0), fold=False,
                 plan=None):
        self.N, self.H, self.W, self.Cin, self.Cout, self.k, self.stride = N, H, W, Cin, Cout, k, stride
        self.fold = fold
        self.KH, self.KW = (k, 1) if fold else (k, k)
        self.ldx = (4 if fold else Cin) if ldx is None else ldx
        self.lddz = Cout if lddz is None else lddz
        self.off, self.pin, self.plan = tuple(off), tuple(pin), plan
        self.OH, self.OW = -(-H // stride), -(-W // stride)
        self.M = N * self.OH * self.OW
        self.n_dw = self.KH * self.KW * Cin * Cout

    def __repr__(self):
        s = "%dx%dx%dx%d->%d k%d s%d" % (self.N, self.H, self.W, self.Cin, self.Cout, self.k, self.stride)
        if self.fold:
            s += " folded"
        if (self.ldx, self.lddz) != (4 if self.fold else self.Cin, self.Cout):
            s += " ldx%d lddz%d" % (self.ldx, self.lddz)
        if any(self.off):
            s += " off%d.%d.%d.%d" % self.off
        if any(self.pin):
            s += " pin%d.%d.%d" % self.pin
        return s

    def but(self, **kw):
        """The same case with some of off / pin / ldx / lddz replaced."""
        a = dict(ldx=self.ldx, lddz=self.lddz, off=self.off, pin=self.pin, fold=self.fold, plan=None)
        a.update(kw)
        return Case(self.N, self.H, self.W, self.Cin, self.Cout, self.k, self.stride, **a)

    @property
    def direct(self):
        return self.M >= DIRECT_MIN_M and not self.fold

    def wplan(self):
        return ops.WgradPlan(self.N, self.H, self.W, self.Cin, self.ldx, self.KH, self.KW, self.stride, self.Cout, self.lddz,
                             fold_cin=4 if self.fold else 0)

    def ws_need(self, slabs):
        return 0 if slabs == 1 else slabs * self.n_dw * 4

    def widths(self, x, dz, dw, ws):
        """(wx, wz) by the rule of max_width: the widest w in {4, 2, 1} that divides the channel count and the leading dimension
        with every pointer involved 4w-aligned -- x for wx; dz for wz, and for the direct kernel also dw and ws, which it stores
        bj floats at a time."""
        def width(c, ld, ptrs):
            for w in (4, 2):
                if c % w == 0 and ld % w == 0 and all(p % (4 * w) == 0 for p in ptrs):
                    return w
            return 1
        return width(self.Cin, self.ldx, [x]), width(self.Cout, self.lddz, [dz, dw, ws] if self.direct else [dz])


def read_plan(lib, case, x, dz, dw, ws):
    """{direct, ai, bj, slabs, wx, wz} of ds_debug_conv_wgrad_plan (the tuning library) for the case at these addresses."""
    out = (C.c_int * 6)()
    rc = lib.ds_debug_conv_wgrad_plan(C.byref(case.wplan().d), C.c_void_p(x), C.c_void_p(dz), case.lddz, C.c_void_p(dw),
                                      C.c_void_p(ws), out)
    assert rc == 0, lib.ds_last_error()
    return tuple(out)


class pinned:
    """with pinned(lib, (ai, bj, slabs)): the plan is pinned inside the block and back at the model's choice after it."""

    def __init__(self, lib, pin):
        self.lib, self.pin = lib, pin

    def __enter__(self):
        assert self.lib.ds_debug_conv_wgrad_force(*self.pin) == 0, self.lib.ds_last_error()

    def __exit__(self, *exc):
        assert self.lib.ds_debug_conv_wgrad_force(0, 0, 0) == 0
        return False


def operands(case, seed, gaussian=False):
    """x [N, H, W, Cin] and dz [N, OH, OW, Cout] in fp64: integers of {-3 .. 3} (every product and partial sum of the kernels is
    then an integer below 2^24, exact in fp32 in any order), or standard normal.  The folded case's x is the [N, H, W, 4] image."""
    rng = np.random.RandomState(seed)
    xs = (case.N, case.H, case.W, 4 if case.fold else case.Cin)
    zs = (case.N, case.OH, case.OW, case.Cout)
    if gaussian:
        return rng.normal(size=xs), rng.normal(size=zs)
    return rng.randint(-3, 4, size=xs).astype(np.float64), rng.randint(-3, 4, size=zs).astype(np.float64)


def reference(case, x, dz):
    """S.conv2d_same_bwd_filter in fp64, [KH, KW, Cin, Cout]; the folded case: the 7 x 7 x 4 filter gradient of the image as
    [7][28][Cout] (tap row, then kw * 4 + channel)."""
    from oracle import tf_semantics as S
    if case.fold:
        return S.conv2d_same_bwd_filter(x, dz, (7, 7, 4, case.Cout), case.stride).reshape(7, 1, 28, case.Cout)
    return S.conv2d_same_bwd_filter(x, dz, (case.k, case.k, case.Cin, case.Cout), case.stride)


# ---- every instantiation x slab form: ragged ci / co tiles at every tile width, ragged wave quarters, an empty last slab at 24
PIN_SHAPES = (Case(3, 14, 13, 40, 72, 3, 1),        # M = 546
              Case(10, 15, 13, 40, 72, 3, 2),       # M = 560, stride 2 with odd extents
              Case(600, 1, 1, 40, 72, 1, 1))        # the GEMM form
PIN_CASES = tuple(c.but(pin=(a, b, s)) for c in PIN_SHAPES for a, b in TILES for s in PIN_SLABS)

# ---- the model's own choices: one shape per tile shape it picks unpinned; Mixed_5c's four launches at batch 32 as they are
# and at batch 256 cut to the smallest batch that keeps the plan of 256 (MIXED_5C_LAYERS: the test asks the library about the
# full batches); and both sides of M = 512.  plan = what ds_debug_conv_wgrad_plan answers for 256-byte aligned operands.
MIXED_5C_LAYERS = ((832, 624, 1), (192, 384, 3), (48, 128, 3), (832, 128, 1))      # (Cin, Cout, k) on the 7 x 7 map
MIXED_5C_BATCHES = (32, 256)
MODEL_CASES = (
    Case(8, 32, 32, 4, 72, 3, 1, plan=(1, 1, 2, 32)),
    Case(4, 32, 32, 4, 384, 3, 1, plan=(1, 1, 4, 16)),
    Case(16, 28, 28, 40, 4, 3, 1, plan=(1, 2, 1, 48)),
    Case(16, 14, 14, 384, 64, 3, 1, plan=(1, 2, 2, 8)),
    Case(2, 16, 16, 384, 1024, 3, 1, plan=(1, 2, 4, 1)),
    Case(4, 32, 32, 384, 4, 3, 1, plan=(1, 4, 1, 16)),
    Case(32, 7, 7, 832, 624, 1, 1, plan=(1, 1, 2, 2)),
    Case(32, 7, 7, 192, 384, 3, 1, plan=(1, 1, 2, 2)),
    Case(32, 7, 7, 48, 128, 3, 1, plan=(1, 1, 1, 4)),
    Case(32, 7, 7, 832, 128, 1, 1, plan=(1, 1, 1, 4)),
    Case(229, 7, 7, 832, 624, 1, 1, plan=(1, 1, 4, 16)),
    Case(44, 7, 7, 192, 384, 3, 1, plan=(1, 1, 4, 4)),
    Case(209, 7, 7, 48, 128, 3, 1, plan=(1, 1, 4, 40)),
    Case(126, 7, 7, 832, 128, 1, 1, plan=(1, 1, 4, 24)),
    Case(73, 7, 1, 24, 40, 1, 1, plan=(0, 0, 0, 8)),          # M = 511: the LDS kernel
    Case(64, 8, 1, 24, 40, 1, 1, plan=(1, 1, 1, 1)),          # M = 512: the direct kernel
)

# ---- an empty trailing slab chosen by the model: 64 slabs of 264 pixels, slab 63 starts behind M
EMPTY_SLAB_CASE = Case(16400, 1, 1, 32, 32, 1, 1, plan=(1, 1, 1, 64))

# ---- operand layouts of the direct kernel
_L = PIN_SHAPES[0]
LAYOUT_CASES = (
    [_L.but(off=(o, 0, 0, 0)) for o in (4, 8)] + [_L.but(ldx=_L.Cin + e) for e in (1, 2, 32)]
    + [_L.but(off=(0, o, 0, 0)) for o in (4, 8)] + [_L.but(lddz=_L.Cout + e) for e in (1, 2, 8)]
    + [_L.but(off=(0, 0, o, 0)) for o in (4, 8)] + [_L.but(off=(0, 0, 0, 8), pin=(0, 0, 4))]
)

# ---- the LDS kernel (M < 512, and the folded stem at any M)
LDS_CASES = (
    Case(2, 15, 13, 12, 20, 3, 2),                              # stride 2, odd extents
    Case(2, 15, 13, 12, 20, 3, 2, ldx=16),
    Case(2, 15, 13, 12, 20, 3, 2, ldx=13),                      # scalar loads of x
    Case(2, 15, 13, 12, 20, 3, 2, lddz=24),
    Case(2, 15, 13, 12, 20, 3, 2, lddz=23),                     # scalar loads of dz
    Case(2, 9, 7, 48, 20, 3, 1),                                # 64-wide ci tiles
    Case(2, 9, 7, 832, 20, 1, 1),                               # 128-wide ci tiles
    Case(2, 23, 21, 28, 24, 7, 2, fold=True),                   # the folded stem, M = 264
    Case(4, 23, 21, 28, 24, 7, 2, fold=True),                   # M = 528: still this kernel
)


def lds_ci_tile(cin):
    """pick_ti of conv_wgrad.hip: 64-wide ci tiles when they cut the padded width by a fifth or more."""
    p128, p64 = -(-cin // 128) * 128, -(-cin // 64) * 64
    return 64 if (p128 - p64) * 5 >= p128 else 128


# ---- taps that never touch the image (no valid output coordinate on an axis), on the direct kernel and, as the control, on
# the LDS kernel; and the double row wrap of OW == 1 without such taps
DEAD_TAP_CASES = (Case(40, 14, 1, 8, 8, 3, 1), Case(40, 1, 14, 8, 8, 3, 1), Case(600, 2, 2, 8, 8, 3, 2), Case(150, 4, 4, 8, 8, 7, 2))
DEAD_TAP_CONTROLS = (Case(30, 14, 1, 8, 8, 3, 1), Case(30, 1, 14, 8, 8, 3, 1), Case(300, 2, 2, 8, 8, 3, 2), Case(100, 4, 4, 8, 8, 7, 2))
DOUBLE_WRAP_CASES = (Case(560, 14, 1, 8, 8, 1, 1), Case(280, 14, 1, 8, 8, 1, 2))


def dead_taps(case):
    """Taps (dh, dw) with no output coordinate o for which o * stride - pad + tap lies inside the image, on either axis."""
    def dead(ext, k, s):
        out = -(-ext // s)
        pad = max((out - 1) * s + k - ext, 0) // 2
        return [t for t in range(k) if not any(0 <= o * s - pad + t < ext for o in range(out))]
    dh, dw = dead(case.H, case.KH, case.stride), dead(case.W, case.KW, case.stride)
    return [(a, b) for a in range(case.KH) for b in range(case.KW) if a in dh or b in dw]


def all_cases():
    return (list(PIN_CASES) + list(MODEL_CASES) + [EMPTY_SLAB_CASE] + LAYOUT_CASES + list(LDS_CASES) + list(DEAD_TAP_CASES)
            + list(DEAD_TAP_CONTROLS) + list(DOUBLE_WRAP_CASES))
