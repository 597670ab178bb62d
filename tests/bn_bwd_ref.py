"""fp64 reference, error bounds and input builders of the batch-statistics BatchNorm + ReLU backward (numpy only).

The backward kernels take mean, rstd, shift (and coef for the apply) as INPUTS, so the reference is the documented formula in
fp64 on those exact fp32 values, for arbitrary vectors:

    g = dy * [z*rstd + shift > 0]        xhat = (z - mean) * rstd
    S1 = sum g, S2 = sum g*xhat          dbeta = S1, coef = (S1/M, S2/M)
    dz = rstd * (g - a1 - xhat*a2)

Every bound below is computed from the inputs (u = 2^-24, the fp32 unit roundoff), never from what a kernel returns:

  column sums    (n + 4) u sum|term|, n the longest fp32 addition chain the launch rule allows.  A term g*xhat carries three
                 roundings (z - mean, * rstd, * g), a chain of n terms n - 1 more: (n + 2) u to first order; the other two units
                 cover the second-order terms (n <= 1024: n^2 u < 0.07) and the cast of a finalized sum to fp32.
  element        6 u rstd (|g| + |a1| + |xhat a2|): dz = rstd * fma(-xhat, a2, g - a1) rounds g - a1 once, xhat twice, the
                 fused multiply-add once and the product with rstd once -- 3 u on |g| + |a1|, 4 u on |xhat a2|.  Behind a
                 pool g itself is a sum of up to four pooled gradients (3 u of the addends' magnitudes): there |g| stands for
                 the sum of the addends' magnitudes, and 3 u + 3 u = 6 u.
  chain          when the device's own coefficients are used, + rstd (|da1| + |xhat| |da2|), da = the sums bound / M.
  bf16 output    + one bf16 ulp of the reference.

The builders keep EVERY element in the comparison (there is no `resolved` mask): `exact` inputs are dyadic, so every fp32
operation of every kernel is exact in any order; `real` inputs have every |z*rstd + shift| >= 2^-10 (asserted to be far above
the rounding of either fp32 spelling of the predicate); `knife` inputs add, in every channel, elements on which the fused and
the unfused fp32 predicate DISAGREE and the fp64 predicate equals the fused one.
"""
import math

import numpy as np

from oracle import tf_semantics as S

U = 2.0 ** -24
MARGIN = 2.0 ** -10

#         M,    C,  ldz, cuts of the dy segments
DENSE = [(1, 4, 4, (0, 4)),
         (3, 16, 20, (0, 16)),
         (1000, 12, 12, (0, 12)),
         (1000, 176, 256, (0, 64, 160, 176)),
         (37, 1024, 1024, (0, 4, 512, 1020, 1024)),
         (8200, 16, 16, (0, 16))]
# the row walk only: C > 1024, and the smallest M at which a thread of the C = 512 launch walks a third row (the grid of the
# streaming kernels stops growing at 16 workgroups per CU = 4096: 8192 rows per step, two rows per pass; the GPU test asserts
# this M against ops.bn_infer_bwd_partials)
LONG_M = 16385
WALK = [(5, 1040, 1040, (0, 1040)),
        (LONG_M, 512, 512, (0, 512))]
KNIFE = [DENSE[2], DENSE[3], DENSE[4]]
#          N, H,  W,  C
POOLED = [(1, 1, 1, 4), (2, 5, 7, 12), (1, 9, 8, 1024), (3, 14, 14, 176)]


def shape_id(s):
    return "%dx%d_ld%d_%dseg" % (s[0], s[1], s[2], len(s[3]) - 1)


def dy_range(M):
    """Largest |dy| of the exact builder: 8, narrowed to 2 for the long case."""
    return 2 if M > 10000 else 8


# ---- number formats -------------------------------------------------------------------------------------------------------
def bf16_round(a):
    """fp32 -> bf16 (round to nearest even) -> fp32."""
    x = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    r = ((x + 0x7FFF + ((x >> 16) & 1)) >> 16) << 16
    return (r & 0xFFFFFFFF).astype(np.uint32).view(np.float32).reshape(np.shape(a))


def bf16_ulp(a):
    """One bf16 ulp at the binade of a (fp64 array)."""
    a = np.abs(np.asarray(a, np.float64))
    e = np.floor(np.log2(np.maximum(a, 2.0 ** -126)))
    return 2.0 ** (e - 7)


def ulps_apart(a, b):
    """Distance of two fp32 arrays in units in the last place (same sign or zero assumed)."""
    ia = np.ascontiguousarray(a, np.float32).view(np.int32).astype(np.int64)
    ib = np.ascontiguousarray(b, np.float32).view(np.int32).astype(np.int64)
    ia = np.where(ia < 0, -(ia & 0x7FFFFFFF), ia)
    ib = np.where(ib < 0, -(ib & 0x7FFFFFFF), ib)
    return np.abs(ia - ib)


# ---- the reference ----------------------------------------------------------------------------------------------------------
class Ref:
    pass


def reference(z, dy, mean, rstd, shift, coef=None, g_mag=None):
    """z, dy [M, C]; mean, rstd, shift [C]; coef [2, C] or None (then the reference's own S1 / M, S2 / M).  g_mag: what stands
    for |g| in the magnitudes (behind a pool: the summed magnitudes of the pooled gradients routed to the pixel)."""
    z, dy = np.asarray(z, np.float64), np.asarray(dy, np.float64)
    mean, rstd, shift = (np.asarray(v, np.float64) for v in (mean, rstd, shift))
    r = Ref()
    r.M = M = z.shape[0]
    r.rstd = rstd
    r.mask = z * rstd + shift > 0
    r.g = np.where(r.mask, dy, 0.0)
    r.xhat = (z - mean) * rstd
    r.S1, r.S2 = r.g.sum(0), (r.g * r.xhat).sum(0)
    ag = np.abs(r.g) if g_mag is None else np.where(r.mask, np.asarray(g_mag, np.float64), 0.0)
    r.A1, r.A2 = ag.sum(0), (ag * np.abs(r.xhat)).sum(0)
    r.dbeta = r.S1
    r.coef = np.stack([r.S1 / M, r.S2 / M])
    r.a1, r.a2 = (r.coef[0], r.coef[1]) if coef is None else (np.asarray(coef[0], np.float64), np.asarray(coef[1], np.float64))
    r.dz = rstd * (r.g - r.a1 - r.xhat * r.a2)
    r.mag = ag + np.abs(r.a1) + np.abs(r.xhat * r.a2)
    return r


# ---- bounds -----------------------------------------------------------------------------------------------------------------
def dense_chain(M):
    """Longest fp32 addition chain of ds_bn_bwd_reduce: a workgroup has at most 512 rows, its LDS combine at most 256 addends."""
    return min(M, 512) + 256


def pooled_chain(patches, C4, P):
    """... of ds_bn_pool_bwd_reduce: a thread meets ceil(patches * C4 / (256 P)) patches of up to four pixels; the combine of
    a workgroup has ceil(256 / C4) <= 256 addends."""
    return 4 * int(math.ceil(patches * C4 / (256.0 * P))) + 256


def sums_tol(n, A):
    return (n + 4) * U * A


def elem_tol(ref):
    return 6 * U * ref.rstd * ref.mag


def chain_extra(ref, n):
    """Propagated error of the device's own coefficients: rstd (|da1| + |xhat| |da2|), da = the sums bound / M."""
    return ref.rstd * (sums_tol(n, ref.A1) / ref.M + np.abs(ref.xhat) * sums_tol(n, ref.A2) / ref.M)


def finalize_tol(ref_value, abs_partials_sum):
    """The finalize kernels add in double and round once: 2^-23 |ref| + 2^-40 sum|partials|."""
    return 2.0 ** -23 * np.abs(ref_value) + 2.0 ** -40 * abs_partials_sum


# ---- builders ---------------------------------------------------------------------------------------------------------------
class Inputs:
    pass


def _pack(mode, z, dy, mean, rstd, shift, coef):
    b = Inputs()
    b.mode = mode
    b.z, b.dy = np.ascontiguousarray(z, np.float32), np.ascontiguousarray(dy, np.float32)
    b.mean, b.rstd, b.shift = (np.ascontiguousarray(v, np.float32) for v in (mean, rstd, shift))
    b.coef = np.ascontiguousarray(coef, np.float32)
    b.knife = np.zeros(b.z.shape, bool)
    b.knife_sign = np.zeros(b.z.shape, np.int8)
    return b


def assert_exact_grid(b):
    """The 2^23 assertion: the column sums of |g| and |g xhat| stay below 2^23 units of the 0.5 grid, so no fp32 partial sum
    of either, in any order, is ever rounded."""
    r = reference(b.z, b.dy, b.mean, b.rstd, b.shift, b.coef)
    for v in (b.z, b.dy, b.mean, 2 * b.rstd, 4 * b.shift, 16 * b.coef, 2 * r.g * r.xhat):
        assert np.array_equal(v, np.round(v))
    assert r.A1.max() < 2.0 ** 22 and r.A2.max() < 2.0 ** 22, (r.A1.max(), r.A2.max())
    assert np.abs(b.z * b.rstd.astype(np.float64) + b.shift).min() >= 0.25


def build_exact(M, C, seed):
    rng = np.random.RandomState(seed)
    d = dy_range(M)
    z = rng.randint(-8, 9, size=(M, C))
    dy = rng.randint(-d, d + 1, size=(M, C))
    mean = rng.randint(-2, 3, size=C)
    rstd = rng.choice([0.5, 1.0, 2.0], size=C)
    shift = rng.randint(-3, 3, size=C) + 0.25
    coef = rng.randint(-32, 33, size=(2, C)) / 16.0
    b = _pack("exact", z, dy, mean, rstd, shift, coef)
    assert_exact_grid(b)
    return b


def assert_margin(b):
    """Every element that is not a knife-edge element decides its ReLU far above the rounding of either fp32 spelling of the
    predicate (an error of at most 2 u (|z rstd| + |shift|)): no element has to be masked out of any comparison."""
    zr = b.z.astype(np.float64) * b.rstd.astype(np.float64)
    t = zr + b.shift
    free = ~b.knife
    assert (np.abs(t[free]) >= MARGIN * (1 - 2.0 ** -8)).all()
    assert (np.abs(t[free]) > 64 * U * (np.abs(zr) + np.abs(b.shift.astype(np.float64)))[free]).all()


def _nudge(z, rstd, shift, skip, to_bf16):
    """z of the elements with |z rstd + shift| < 2^-10 moved to the nearest fp32 value that puts it at +-2^-10 (on the bf16
    grid: one bf16 step at a time, away from the edge, until it is out)."""
    r64, s64 = rstd.astype(np.float64), shift.astype(np.float64)
    z = z.copy()
    t = z.astype(np.float64) * r64 + s64
    bad = (np.abs(t) < MARGIN) & ~skip
    if not bad.any():
        return z
    side = np.where(t >= 0, 1.0, -1.0)
    if not to_bf16:
        target = ((side * MARGIN * (1 + 2.0 ** -12) - s64) / r64).astype(np.float32)
        z[bad] = target[bad]
        return z
    # (to the bf16 value next to the fp32 target first, then single steps)
    target = bf16_round(((side * MARGIN * (1 + 2.0 ** -6) - s64) / r64).astype(np.float32))
    z[bad] = target[bad]
    t = z.astype(np.float64) * r64 + s64
    bad = (np.abs(t) < MARGIN) & ~skip
    if not bad.any():
        return z
    for _ in range(64):
        step =np.spacing(np.maximum(np.abs(z), np.float32(2.0 ** -30))).astype(np.float64) * 65536.0
        moved = bf16_round((z.astype(np.float64) + side * step).astype(np.float32))
        z[bad] = moved[bad]
        t = z.astype(np.float64) * r64 + s64
        bad = (np.abs(t) < MARGIN) & ~skip
        if not bad.any():
            return z
    raise AssertionError("the nudge did not leave the edge")


def build_real(M, C, seed, z_bf16=False, nudge=True, integer_dy=False):
    """Normal z and dy; mean, rstd, shift from the oracle's S.batch_norm_train (fp64), rounded to fp32.  z_bf16: z is rounded
    to bf16 first."""
    rng = np.random.RandomState(seed)
    z = (rng.normal(size=(M, C)) * rng.uniform(0.5, 2.0, size=C) + rng.normal(size=C)).astype(np.float32)
    if z_bf16:
        z = bf16_round(z)
    beta = rng.normal(0, 0.3, size=C)
    _, mean, _, _, rstd = S.batch_norm_train(z.astype(np.float64), beta)
    mean, rstd = mean.astype(np.float32), rstd.astype(np.float32)
    shift = (beta - mean.astype(np.float64) * rstd).astype(np.float32)
    dy = rng.randint(1, 9, size=(M, C)) if integer_dy else rng.normal(size=(M, C))
    coef = rng.normal(0, 0.1, size=(2, C))
    b = _pack("real", z, dy, mean, rstd, shift, coef)
    b.beta = beta
    if nudge:
        b.z = _nudge(b.z, b.rstd, b.shift, b.knife, z_bf16)
        assert_margin(b)
        if z_bf16:
            assert np.array_equal(b.z, bf16_round(b.z))
    return b


def knife_candidates(r, s):
    """fp32 z with fl(z * r) == -s exactly and z * r != -s: the unfused fp32 predicate fl(fl(z r) + s) > 0 is false there, the
    fused one has the sign of the rounding residual z r + s (exact in fp64: a 48-bit product, then a cancelling sum).  Searched
    over fl(-s / r) + k ulp, |k| <= 2.  Returns (z values with a positive residual, ... with a negative one)."""
    r64, s64 = float(r), float(s)
    z0 = np.float32(-s64 / r64)
    pos, neg = [], []
    for k in range(-2, 3):
        zk = z0
        for _ in range(abs(k)):
            zk = np.nextafter(zk, np.float32(np.inf if k > 0 else -np.inf))
        p = float(zk) * r64
        if np.float32(p) == np.float32(-s64) and p != -s64:
            (pos if p + s64 > 0 else neg).append(zk)
    return pos, neg


def build_knife(M, C, seed):
    """`real` (integer dy in [1, 8]: a changed mask changes sum g by an integer) with a quarter of the elements of every channel
    replaced by knife-edge values, alternately of positive and negative residual.  rstd of a channel is redrawn until the
    channel has a candidate of either sign; the statistics are inputs, so nothing else depends on that."""
    b = build_real(M, C, seed, nudge=False, integer_dy=True)
    b.mode = "knife"
    rng = np.random.RandomState(seed + 7919)
    nk = -(-M // 4)
    for c in range(C):
        r0, s = b.rstd[c], b.shift[c]
        assert s != 0
        # two neighbouring z can round onto -shift only where the product's ulp is finer than shift's: where rstd's
        # significand m_r exceeds shift's m_s, and then with a probability of about 2 / m_r - 1.  The redraws keep rstd's
        # binade and draw the significand from (m_s, 2).  A shift with m_s so close to 2 that 20000 draws find nothing is
        # scaled by 3/4 (it is an input like the others).
        e = math.floor(math.log2(float(r0)))
        r, pos, neg = r0, [], []
        for _ in range(8):
            ms = 2 * math.frexp(abs(float(s)))[0]
            for _ in range(20000):
                pos, neg = knife_candidates(r, s)
                if pos and neg:
                    break
                r = np.float32(rng.uniform(ms, 2.0) * 2.0 ** e)
            if pos and neg:
                break
            s = np.float32(0.75 * s)
        else:
            raise AssertionError("no knife-edge pair for channel %d" % c)
        b.rstd[c], b.shift[c] = r, s
        rows = rng.permutation(M)[:nk]
        sign = np.where(np.arange(nk) % 2 == 0, 1, -1)
        vals = np.where(sign > 0, np.asarray(pos, np.float32)[rng.randint(len(pos), size=nk)],
                        np.asarray(neg, np.float32)[rng.randint(len(neg), size=nk)])
        b.z[rows, c] = vals
        b.knife[rows, c] = True
        b.knife_sign[rows, c] = sign
    b.z = _nudge(b.z, b.rstd, b.shift, b.knife, False)
    assert_margin(b)
    return b


_CACHE = {}


def build(mode, M, C, seed=0, z_bf16=False):
    """Cached (a reference is computed once and shared; callers do not modify what they get)."""
    key = (mode, M, C, seed, z_bf16 and mode == "real")
    if key not in _CACHE:
        if mode == "exact":
            _CACHE[key] = build_exact(M, C, 1000 + seed)
        elif mode == "real":
            _CACHE[key] = build_real(M, C, 2000 + seed, z_bf16)
        else:
            _CACHE[key] = build_knife(M, C, 3000 + seed)
    return _CACHE[key]


# ---- behind a 3x3 / 2 SAME max pool -------------------------------------------------------------------------------------------
def window_maxima_are_unique(z):
    """No 3x3 / 2 SAME window of z [N, H, W, C] has its maximum twice (the winners do not depend on a tie rule)."""
    win, _, _ = S._patches(np.asarray(z, np.float64), 3, 3, 2, -np.inf, "SAME")
    n, oh, ow = win.shape[:3]
    flat = win.reshape(n, oh, ow, 9, -1)
    return bool(((flat == flat.max(axis=3, keepdims=True)).sum(axis=3) == 1).all())


def build_pooled(mode, N, H, W, C, seed=0):
    """Inputs of the pooled twins: z [N, H, W, C] and the POOLED gradient dpool [N, OH, OW, C]; b.dy is the oracle's
    S.max_pool_bwd of it (fp64) and b.dy_mag the same routing of |dpool|.  exact: z = a per-(sample, channel) choice of nine
    distinct integers of [-8, 8] laid out by (h mod 3, w mod 3), so the pixels of any 3x3 window are all different."""
    key = ("pool", mode, N, H, W, C, seed)
    if key in _CACHE:
        return _CACHE[key]
    M = N * H * W
    OH, OW = -(-H // 2), -(-W // 2)
    b = build(mode, M, C, seed + 50)
    p = Inputs()
    p.__dict__.update(b.__dict__)
    rng = np.random.RandomState(4000 + seed + M + C)
    if mode == "exact":
        vals = np.argsort(rng.uniform(size=(N, C, 17)), axis=2)[:, :, :9] - 8          # nine distinct integers per (n, c)
        hh, ww = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        slot = (hh % 3) * 3 + (ww % 3)
        z4 = np.transpose(vals[:, :, slot], (0, 2, 3, 1)).astype(np.float32)
        dpool = rng.randint(-8, 9, size=(N, OH, OW, C)).astype(np.float32)
    else:
        z4 = b.z.reshape(N, H, W, C)
        dpool = rng.normal(size=(N, OH, OW, C)).astype(np.float32)
    assert window_maxima_are_unique(z4)
    p.z4, p.z = z4, z4.reshape(M, C)
    p.dpool = dpool
    p.dy = S.max_pool_bwd(z4.astype(np.float64), dpool.astype(np.float64), 3, 2).reshape(M, C)
    p.dy_mag = S.max_pool_bwd(z4.astype(np.float64), np.abs(dpool).astype(np.float64), 3, 2).reshape(M, C)
    p.winners = S.max_pool_argmax(z4.astype(np.float64), 3, 2)
    p.patches = N * (OH + 1) * (OW + 1)
    if mode == "exact":
        assert_exact_grid(_pack("exact", p.z, p.dy, p.mean, p.rstd, p.shift, p.coef))      # (dy: up to four integers per pixel)
    else:
        assert_margin(p)
    _CACHE[key] = p
    return p
