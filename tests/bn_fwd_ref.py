"""fp64 reference, derived gates, case tables and checks of the BatchNorm FORWARD kernels of csrc/bn.hip (numpy only):
ds_bn_finalize / _centered / _multi, ds_bn_apply_relu / _z16, ds_bn_infer_prepare / _multi.

The reference restates each kernel from the fp32 values the kernel itself reads (partials, z, rstd, shift, moving vectors):

    finalize   s, q = sum of the partials [2][C][P];  du = s / count;  mu = du + pivot;  var = max(q / count - du^2, 0)
               rstd = 1 / sqrt(var + eps);  shift = beta - mu rstd;  mean_c = du;  shift_c = beta - du rstd
               moving <- decay moving + (1 - decay) batch                        (S.batch_norm_moving_update)
    apply      y = max(z rstd + shift, 0), scattered into up to four column segments (fp32 or bf16 RNE), max(y) per segment
    infer      rstd = 1 / sqrt(moving_var + eps);  shift = beta - moving_mean rstd

Every gate is derived (U32 = one fp32 ulp of the value in question), none is picked from what a kernel returns:

  * the kernel combines the partials in double and casts once.  mean, mean_c, rstd and the fp32 cast of var are gated at ONE
    ulp32 of the reference: half for the cast, the other half is room for the order of the double sums.  Where the double
    arithmetic itself cancels, the room is computed per channel and added:
      - rstd: 2^-50 (q/count) / (var + eps), relative -- the cancellation of q/count - du^2;
      - var:  2^-47 (q/count), absolute.  The kernel's sum tree is 8 strided adds + 6 butterfly levels + 3 waves = 17 deep, two
        more roundings scale by 1/count: 19 x 2^-53 on q/count, twice that on du^2 <= q/count (Cauchy-Schwarz on the partials),
        two for the square and the difference: 59 x 2^-53 < 2^-47.  (The reference adds with math.fsum and forms
        q/count - du^2 in exact rational arithmetic, so it contributes nothing.)
      - mean, mean_c: 2^-47 sum|s_p| / count, absolute (the same tree).
  * shift, shift_c and the moving updates are fp32 EXPRESSIONS the compiler may or may not contract into an fma.  Their gate is
    the first-order rounding bound of the expression as written -- half an ulp32 of each intermediate product plus half an
    ulp32 of the result -- evaluated in fp64 from the kernel's OWN fp32 mean / rstd / var (already checked above), so both
    contractions pass.  A product or sum that is exactly representable in fp32 rounds in neither form and contributes 0: that
    is what makes an exact zero, a decay of 0 and a bf16 tie exact checks.  The result's ulp is taken at |t| + the products'
    bound, so a result pushed over a binade edge by a product's rounding is covered.
  * apply: the same bound b for t = z rstd + shift, absolute; max(., 0) moves no two numbers apart, so |y - max(t, 0)| <= b
    holds through the ReLU kink and no element is masked out.  With lo = max(t - b, 0) and hi = max(t + b, 0), a bf16
    destination must lie in [bf16_rne(lo), bf16_rne(hi)] (rounding is monotone) and a record in [max lo, max hi] of its
    segment.
  * infer prepare: see infer_rstd_gate -- the documented ulp errors of the add, sqrtf and the division under the flags the
    library is compiled with.

The checks (check_finalize, check_apply, check_infer) take host arrays, so tests/test_bn_fwd_ref_cpu.py runs them on NumPy
emulations of the kernels (either contraction, planted defects) and tests/test_bn_fwd_gpu.py on what the device wrote.
"""
import math
from fractions import Fraction

import numpy as np

from conv_check import bf16_round
from oracle import tf_semantics as S

F32 = np.float32
EPS = F32(S.BN_EPS)
DECAY = F32(S.BN_DECAY)
SENT = -777.25            # outputs are ReLU outputs or sit in vectors built to stay away from it
SENT16 = -776.0           # the same for a bf16 tensor (exactly representable there)
GUARD = 64
DT_F32, DT_BF16 = 0, 1    # (DS_DTYPE_F32 / DS_DTYPE_BF16: asserted against ops by the GPU module)
AMAX_FLOATS = 512         # a max record: 16 slots, one per 128-byte line (ops.AMAX_FLOATS)
KCUS, BPC = 256, 16       # ds::kCUs and the streaming kernels' workgroups per CU (column_grid in bn.hip)


# ---- number formats -----------------------------------------------------------------------------------------------------------
def ulp32(x):
    """One fp32 unit in the last place at |x| (x in fp64; the subnormal step below the smallest normal)."""
    m = np.maximum(np.abs(np.asarray(x, np.float64)), 2.0 ** -126)
    return np.ldexp(1.0, np.frexp(m)[1] - 24)


def half_ulp_unless_exact(x):
    """The rounding error bound of an fp32 operation whose exact result is x: 0 where x is an fp32 number."""
    x = np.asarray(x, np.float64)
    return np.where(x.astype(F32).astype(np.float64) == x, 0.0, 0.5 * ulp32(x))


def product_sum_gate(p, t):
    """Bound of fl(fl(p) + c) or fma(.., .., c) where p is the exact product and t = p + c the exact result."""
    bp = half_ulp_unless_exact(p)
    t = np.asarray(t, np.float64)
    exact = (bp == 0) & (t.astype(F32).astype(np.float64) == t)
    return bp + np.where(exact, 0.0, 0.5 * ulp32(np.abs(t) + bp))


def two_product_gate(p1, p2):
    """Bound of a p1 + p2 expression with two fp32 products (either may be the fma's)."""
    b1, b2 = half_ulp_unless_exact(p1), half_ulp_unless_exact(p2)
    t = np.asarray(p1, np.float64) + np.asarray(p2, np.float64)
    exact = (b1 == 0) & (b2 == 0) & (t.astype(F32).astype(np.float64) == t)
    return b1 + b2 + np.where(exact, 0.0, 0.5 * ulp32(np.abs(t) + b1 + b2))


class Report(dict):
    """name -> largest error / gate seen; check() raises when one exceeds 1."""

    def add(self, name, err, gate):
        err = np.abs(np.asarray(err, np.float64))
        gate = np.broadcast_to(np.asarray(gate, np.float64), err.shape)
        if err.size == 0:
            return
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(gate > 0, err / np.where(gate > 0, gate, 1.0), np.where(err > 0, np.inf, 0.0))
        r = np.where(np.isfinite(err), r, np.inf)
        self[name] = max(self.get(name, 0.0), float(r.max()))

    def require(self, name, ok):
        self[name] = max(self.get(name, 0.0), 0.0 if ok else np.inf)

    def merge(self, other):
        for k, v in other.items():
            self[k] = max(self.get(k, 0.0), v)
        return self

    def table(self):
        """Per entry point (the part of a name before the colon): the largest error / gate of each of its checks."""
        lines = []
        for k in sorted(self):
            who, _, item = k.partition(":")
            lines.append("  %-28s %-52s %.3f" % (who, item, self[k]))
        return "\n".join(lines)

    def failed(self):
        return sorted(k for k, v in self.items() if not v <= 1.0)

    def check(self):
        assert not self.failed(), "outside the gate: %s" % ", ".join("%s (%.3g)" % (k, self[k]) for k in self.failed())
        return self


# ---- the launch rule of the streaming kernels -----------------------------------------------------------------------------------
def column_grid(M, C):
    """(grid, drow) of ds_bn_apply_relu: the grid is a multiple of C4 / gcd(C4, 256), capped at kCUs * 16 workgroups (rounded
    up to the granule), sized for two rows per thread and pass; drow = grid * 256 / C4 rows are in flight at once."""
    C4 = C // 4
    q = C4 // math.gcd(C4, 256)
    want = min((M * C4 + 511) // 512, KCUS * BPC)
    k = max((want + q - 1) // q, 1)
    grid = k * q
    assert grid * 256 % C4 == 0
    return grid, grid * 256 // C4


def rows_per_thread(M, C):
    """(most, fewest) rows among the threads that have any: thread row0 walks row0, row0 + drow, ..."""
    _, drow = column_grid(M, C)
    most = -(-M // drow)
    fewest = most if M % drow == 0 or M < drow else most - 1
    return most, max(fewest, 1)


# ---- finalize -------------------------------------------------------------------------------------------------------------------
#            P,    C,   count,           pivot,   (mm, mv), decay, centered
BIG = 256 * 112 * 112
FINALIZE = [(1, 4, 1, "none", (True, True), DECAY, False),
            (63, 176, 3000, "sep", (True, True), DECAY, True),
            (64, 1024, 64, "alias", (True, False), F32(0), False),
            (255, 4, BIG, "none", (False, True), DECAY, True),
            (256, 176, 3000, "sep", (False, False), DECAY, False),
            (257, 4, 257, "none", (True, True), DECAY, False),
            (257, 176, 3000, "sep", (True, False), DECAY, True),
            (257, 1024, 3000, "alias", (False, False), F32(0), True),
            (700, 1024, 700, "none", (False, True), DECAY, False),
            (700, 4, BIG, "sep", (True, True), F32(0), True),
            (700, 176, 3000, "alias", (True, True), DECAY, False),
            (2048, 4, BIG, "none", (True, True), DECAY, True),
            (2048, 176, 3000, "sep", (False, True), DECAY, False),
            (2048, 1024, 2048, "alias", (True, True), DECAY, True)]
# ds_bn_finalize_multi: 1..4 jobs (C = 4 beside C = 832, P = 1 beside P > 256, null moving vectors beside real ones); the
# pivot of an "alias" job is its slice of the launch's concatenated mean vector
FINALIZE_MULTI = [(DECAY, [(300, 12, 3000, "sep", (True, True))]),
                  (DECAY, [(1, 4, 1, "none", (True, True)), (700, 832, 3000, "alias", (False, False))]),
                  (F32(0), [(24, 64, 3000, "none", (True, True)), (257, 4, 257, "sep", (True, False)),
                            (7, 176, 1000, "alias", (False, True))]),
                  (DECAY, [(130, 176, 3000, "alias", (True, True)), (1, 4, 5, "alias", (False, False)),
                           (2048, 12, 2048, "none", (True, True)), (63, 832, 3000, "sep", (False, True))])]


def fin_id(c):
    return "P%d_C%d_n%d_%s_mm%d_mv%d_d%g%s" % (c[0], c[1], c[2], c[3], c[4][0], c[4][1], float(c[5]), "_centered" if c[6] else "")


class Case:
    pass


_CACHE = {}
FIFTY, CONST, CLAMP = 0, 1, 2          # the special channels of every finalize case


def fifty_sigma_channels(C):
    return [c for c in range(C) if c == FIFTY or (c % 16 == 5 and C > 4)]


def build_finalize(P, C, count, pivot, moving, decay=DECAY, centered=False, seed=0):
    """Partials of a real fp32 z [count, C]: the sums of (z - pivot) and (z - pivot)^2 over P row chunks, in fp64, cast to
    fp32.  Channels: FIFTY (and every 16th from 5) have |mean| = 50 sigma, CONST is constant, CLAMP is constant with its q
    partials scaled by 1 - 2^-20, which makes q/count - du^2 slightly negative (asserted on the reference)."""
    key = ("fin", P, C, count, pivot, moving, float(decay), centered, seed)
    if key in _CACHE:
        return _CACHE[key]
    assert count >= P and C >= 4
    rng = np.random.RandomState(100 + seed + P + 7 * C)
    sigma = rng.uniform(0.5, 2.0, size=C)
    mean = rng.normal(size=C)
    for c in fifty_sigma_channels(C):
        mean[c] = 50.0 * sigma[c] * (-1 if c % 32 else 1)
    z = (rng.standard_normal(size=(count, C)).astype(F32) * sigma.astype(F32) + mean.astype(F32)).astype(F32)
    z[:, CONST], z[:, CLAMP] = F32(1.7), F32(-2.3)
    zmean = z.mean(axis=0, dtype=np.float64)
    k = Case()
    k.P, k.C, k.count, k.pivot_kind, k.moving, k.decay, k.centered = P, C, count, pivot, moving, F32(decay), centered
    k.eps = EPS
    k.pivot = {"none": None, "sep": (zmean + 0.5 * sigma).astype(F32), "alias": (zmean + 0.01 * sigma).astype(F32)}[pivot]
    u = z.astype(np.float64)
    del z
    if k.pivot is not None:
        u -= k.pivot.astype(np.float64)
    cuts = (np.arange(P, dtype=np.int64) * count) // P            # P chunks of at least one row
    s = np.add.reduceat(u, cuts, axis=0)
    u *= u
    q = np.add.reduceat(u, cuts, axis=0)
    del u
    q[:, CLAMP] *= 1.0 - 2.0 ** -20
    k.stats = np.ascontiguousarray(np.stack([s.T, q.T]), F32)      # [2][C][P]
    k.beta = rng.normal(0, 0.3, size=C).astype(F32)
    k.mm0 = rng.normal(size=C).astype(F32)
    k.mv0 = rng.uniform(0.5, 2.0, size=C).astype(F32)
    k.ref = finalize_ref(k.stats, count, k.pivot, k.beta, k.eps)
    assert k.ref.var_raw[CLAMP] < 0 and k.ref.var[CLAMP] == 0 and k.ref.rstd[CLAMP] == 1.0 / math.sqrt(float(EPS))
    for c in fifty_sigma_channels(C):
        if count >= 1000:
            assert 40 < abs(k.ref.mu[c]) * k.ref.rstd[c] < 60
    _CACHE[key] = k
    return k


def finalize_ref(stats, count, pivot, beta, eps):
    """The fp64 restatement.  s and q are math.fsum of the fp32 partials (correctly rounded sums) and q/count - du^2 is formed
    in exact rational arithmetic before it is rounded to fp64: the reference adds no cancellation of its own."""
    stats = np.asarray(stats, F32)
    C = stats.shape[1]
    r = Case()
    st = stats.astype(np.float64)
    r.s = np.array([math.fsum(st[0, c]) for c in range(C)])
    r.q = np.array([math.fsum(st[1, c]) for c in range(C)])
    r.abs_s = np.abs(st[0]).sum(axis=1)
    r.du = r.s / count
    r.var_raw = np.array([float(Fraction(float(r.q[c])) / count - (Fraction(float(r.s[c])) / count) ** 2) for c in range(C)])
    r.qmean = r.q / count
    r.var = np.maximum(r.var_raw, 0.0)
    r.mu = r.du + (0.0 if pivot is None else np.asarray(pivot, np.float64))
    r.rstd = 1.0 / np.sqrt(r.var + float(eps))
    b = np.asarray(beta, np.float64)
    r.shift, r.mean_c, r.shift_c = b - r.mu * r.rstd, r.du, b - r.du * r.rstd
    # the gates of the values that come out of the double arithmetic
    r.g_mean = ulp32(r.mu) + 2.0 ** -47 * r.abs_s / count
    r.g_mean_c = ulp32(r.du) + 2.0 ** -47 * r.abs_s / count
    r.g_var = ulp32(r.var) + 2.0 ** -47 * r.qmean
    r.g_rstd = ulp32(r.rstd) + r.rstd * 2.0 ** -50 * r.qmean / (r.var + float(eps))
    return r


def shift_gate(beta, m32, r32):
    """(t, gate) of the fp32 expression beta - m * r from the fp32 operands."""
    p = np.asarray(m32, np.float64) * np.asarray(r32, np.float64)
    t = np.asarray(beta, np.float64) - p
    return t, product_sum_gate(p, t)


def moving_gate(decay, old, batch32):
    """(t, gate) of decay * old + (1.f - decay) * batch; 1.f - decay is exact in fp32 for a decay in [0.5, 1] and for 0."""
    d = float(F32(decay))
    omd = float(F32(1) - F32(decay))
    assert omd == 1.0 - d
    p1, p2 = d * np.asarray(old, np.float64), omd * np.asarray(batch32, np.float64)
    return p1 + p2, two_product_gate(p1, p2)


def check_finalize(k, got, probe, what="finalize"):
    """got: the case's launch (mean, rstd, shift, [mean_c, shift_c], [mm], [mv]); probe: a launch of the same partials with
    decay = 0 and both moving vectors, whose mv IS the kernel's fp32 cast of var and whose mm is its mean.  Every output is
    float32 [C]; a vector the case passes as null must be absent from got."""
    ref, rep = k.ref, Report()
    f = lambda a: np.asarray(a, np.float64)
    for name in ("mean", "rstd", "shift"):
        assert np.asarray(got[name]).dtype == F32 and np.asarray(probe[name]).dtype == F32
        rep.require(what + ":probe repeats " + name, np.array_equal(np.asarray(got[name]).view(np.uint32),
                                                                   np.asarray(probe[name]).view(np.uint32)))
    var32 = np.asarray(probe["mv"], F32)
    rep.require(what + ":decay 0 stores the mean", np.array_equal(np.asarray(probe["mm"]).view(np.uint32),
                                                                 np.asarray(got["mean"]).view(np.uint32)))
    rep.add(what + ":mean", f(got["mean"]) - ref.mu, ref.g_mean)
    rep.add(what + ":rstd", f(got["rstd"]) - ref.rstd, ref.g_rstd)
    rep.add(what + ":var", f(var32) - ref.var, ref.g_var)
    rep.require(what + ":clamp", var32[CLAMP] == 0 and got["rstd"][CLAMP] == F32(1.0 / math.sqrt(float(k.eps))))
    t, g = shift_gate(k.beta, got["mean"], got["rstd"])
    rep.add(what + ":shift", f(got["shift"]) - t, g)
    if k.centered:
        rep.add(what + ":mean_c", f(got["mean_c"]) - ref.mean_c, ref.g_mean_c)
        t, g = shift_gate(k.beta, got["mean_c"], got["rstd"])
        rep.add(what + ":shift_c", f(got["shift_c"]) - t, g)
    else:
        assert "mean_c" not in got and "shift_c" not in got
    omd = float(F32(1) - k.decay)
    want_mm, want_mv = S.batch_norm_moving_update(f(k.mm0), f(k.mv0), ref.mu, ref.var, float(k.decay))
    for name, has, old, batch32, want, g_batch in (("mm", k.moving[0], k.mm0, got["mean"], want_mm, ref.g_mean),
                                                   ("mv", k.moving[1], k.mv0, var32, want_mv, ref.g_var)):
        if not has:
            assert name not in got
            continue
        t, g = moving_gate(k.decay, old, batch32)
        rep.add(what + ":" + name, f(got[name]) - t, g)
        # ... and end to end against the oracle's update of the reference's statistics
        rep.add(what + ":" + name + " (oracle)", f(got[name]) - want, g + omd * g_batch)
    return rep.check()


# ---- apply ----------------------------------------------------------------------------------------------------------------------
# buffers: (ld, dtype) of every destination tensor [M, ld]; segments, IN LAUNCH ORDER: (c0, c1, buffer, first column there,
# record?, all-negative?)
def _layout(M, C):
    if C == 4:
        return [(4, DT_F32)], [(0, 4, 0, 0, True, False)]
    if C == 12:          # three segments, mixed storage, a record on the middle one only
        return [(8, DT_F32), (4, DT_BF16), (12, DT_F32)], [(0, 4, 0, 4, False, False), (4, 8, 1, 0, True, False),
                                                            (8, 12, 2, 8, False, False)]
    if C == 176:         # 64 | 96 | 16: the first and the last into one wider concat row, the middle on its own
        return [(256, DT_F32), (100, DT_BF16)], [(0, 64, 0, 32, True, False), (64, 160, 1, 0, True, False),
                                                 (160, 176, 0, 200, False, False)]
    if C == 1024:        # four segments out of channel order; the cuts fall inside a wave; records on two; one all-negative
        return ([(156, DT_F32), (104, DT_BF16), (448, DT_F32), (324, DT_BF16)],
                [(256, 700, 2, 4, True, False), (0, 100, 1, 4, False, False), (700, 1024, 3, 0, True, True),
                 (100, 256, 0, 0, False, False)])
    if C == 1000:        # C4 = 250: the cut at column group 125 is in the middle of every second wave; a record on one side
        return [(500, DT_BF16), (512, DT_F32)], [(500, 1000, 1, 8, False, False), (0, 500, 0, 0, True, False)]
    if C == 832:         # four segments in order, all-negative fp32 segment with a record, bf16 all-negative without
        return ([(208, DT_F32), (208, DT_BF16), (212, DT_F32), (208, DT_BF16)],
                [(0, 208, 0, 0, True, True), (208, 416, 1, 0, True, False), (416, 624, 2, 4, False, False),
                 (624, 832, 3, 0, False, True)])
    if C == 64 and M > 150000:
        return [(32, DT_F32), (32, DT_BF16)], [(0, 32, 0, 0, True, False), (32, 64, 1, 0, True, False)]
    if C == 64:
        return [(64, DT_F32)], [(0, 64, 0, 0, True, False)]
    raise KeyError((M, C))


APPLY = [(1, 4), (1, 1024), (7, 12), (255, 1000), (1001, 832), (777, 176), (140001, 64), (196685, 64)]
APPLY_Z16 = APPLY[:-1]
LONG_ONE_ROW_TAIL, LONG_SOME_ROWS_TAIL = APPLY[6], APPLY[7]


def apply_id(s):
    return "%dx%d" % s


def build_apply(M, C, z16=False, seed=0):
    """z [M, C] (bf16-exact when z16), rstd, shift and the reference interval.  Planted in z: exact zeros; in the channels
    c % 8 == 3 values at and next to fl(-shift / rstd) (the ReLU kink); in the channels c % 8 == 1 (rstd = 0.5, shift = 0.25
    there) values whose z rstd + shift is exactly halfway between two bf16 numbers."""
    key = ("apply", M, C, z16, seed)
    if key in _CACHE:
        return _CACHE[key]
    rng = np.random.RandomState(300 + seed + M % 1000 + C)
    k = Case()
    k.M, k.C, k.z16 = M, C, z16
    k.buffers, k.segs = _layout(M, C)
    k.rstd = rng.uniform(0.5, 2.0, size=C).astype(F32)
    k.shift = rng.normal(0, 0.5, size=C).astype(F32)
    tie_c = np.arange(C) % 8 == 1
    kink_c = np.arange(C) % 8 == 3
    for (c0, c1, _, _, _, neg) in k.segs:          # an all-negative segment: z rstd + shift < -80 everywhere
        if neg:
            k.shift[c0:c1] = F32(-100.0)
            tie_c[c0:c1] = kink_c[c0:c1] = False
    k.rstd[tie_c], k.shift[tie_c] = F32(0.5), F32(0.25)
    z = rng.standard_normal(size=(M, C)).astype(F32)
    rows = np.arange(M)[:, None]
    cols = np.arange(C)[None, :]
    # the kink: fl(-s / r) and its two fp32 neighbours, cycling down the rows
    kink = kink_c[None, :] & np.ones((M, 1), bool)
    z0 = (-(k.shift.astype(np.float64)) / k.rstd.astype(np.float64)).astype(F32)
    near = np.stack([np.nextafter(z0, F32(-np.inf)), z0, np.nextafter(z0, F32(np.inf))])
    z = np.where(kink, near[(rows % 3), cols], z)
    # bf16 ties: t = (1 + j / 128 + 1 / 256) * 2^e, j = 0 .. 127, e in {-1, 0, 1}; z = (t - 0.25) * 2 is an fp32 number
    j = (rows * 5 + cols) % 128
    e = (rows + cols // 8) % 3 - 1
    tie = (1.0 + j / 128.0 + 1.0 / 256.0) * 2.0 ** e
    z = np.where(tie_c[None, :] & np.ones((M, 1), bool), ((tie - 0.25) * 2.0).astype(F32), z).astype(F32)
    z[(rows * 7 + cols * 3) % 11 == 0] = F32(0)
    if z16:          # (a tie needs more than 8 significant bits of z: the z16 form keeps the exact zeros and the exact channels)
        z = bf16_round(z).astype(F32)
    k.z = np.ascontiguousarray(z, F32)
    p = k.z.astype(np.float64) * k.rstd.astype(np.float64)
    t = p + k.shift.astype(np.float64)
    b = product_sum_gate(p, t)
    k.lo, k.hi = np.maximum(t - b, 0.0), np.maximum(t + b, 0.0)
    k.t, k.b = t, b
    if not z16:
        tied = tie_c[None, :] & (k.z != 0)
        assert tied.any() and (b[tied] == 0).all()
        assert (bf16_round(t[tied].astype(F32)) != t[tied]).all()                    # not bf16 numbers ...
        up, dn = bf16_round((t[tied] * (1 + 2.0 ** -12)).astype(F32)), bf16_round((t[tied] * (1 - 2.0 ** -12)).astype(F32))
        assert np.allclose(up - t[tied], t[tied] - dn, rtol=0, atol=0)                # ... but exactly between two of them
    assert ((k.z == 0).sum() > 0) or M * C < 11
    _CACHE[key] = k
    return k


def empty_buffers(k):
    """The destination tensors, full of sentinels, and the records: 0 in the 16 slot words, sentinels between them."""
    bufs = [np.full((k.M, ld), SENT if dt == DT_F32 else SENT16, F32) for ld, dt in k.buffers]
    recs = []
    for seg in k.segs:
        r = np.full(AMAX_FLOATS, SENT, F32)
        r[::32] = 0
        recs.append(r if seg[4] else None)
    return bufs, recs


def check_apply(k, bufs, recs, what="apply"):
    """bufs: the destination tensors as float32 [M, ld] (a bf16 tensor widened exactly); recs: per segment the AMAX_FLOATS
    words of its record, or None."""
    rep = Report()
    written = [np.zeros((k.M, ld), bool) for ld, _ in k.buffers]
    for i, (c0, c1, bi, col, has_rec, neg) in enumerate(k.segs):
        dt = k.buffers[bi][1]
        got = np.asarray(bufs[bi], F32)[:, col:col + c1 - c0].astype(np.float64)
        assert not written[bi][:, col:col + c1 - c0].any()
        written[bi][:, col:col + c1 - c0] = True
        lo, hi = k.lo[:, c0:c1], k.hi[:, c0:c1]
        kind = "fp32" if dt == DT_F32 else "bf16"
        if dt == DT_BF16:
            lo_s, hi_s = bf16_round(lo.astype(F32)), bf16_round(hi.astype(F32))
            rep.require("%s:%s exact interval" % (what, kind), bool(((got >= lo_s) & (got <= hi_s)).all()))
        # max(., 0) moves no two numbers apart, so |y - max(t, 0)| <= b holds through the kink; behind the (monotone) bf16
        # rounding half a bf16 ulp more -- that ratio is reported, the interval above is the bf16 check
        y, b = np.maximum(k.t[:, c0:c1], 0.0), k.b[:, c0:c1]
        half16 = 2.0 ** (np.ceil(np.log2(np.maximum(hi, 2.0 ** -126))) - 9)          # half a bf16 ulp of anything <= hi
        rep.add("%s:%s y" % (what, kind), got - y, b if dt == DT_F32 else b + half16)
        if has_rec:
            r = np.asarray(recs[i], F32)
            slots, rest = r[::32], np.delete(r, np.arange(0, AMAX_FLOATS, 32))
            rep.require(what + ":record words between the slots", bool((rest == F32(SENT)).all()))
            v = float(slots.max())
            rep.require(what + ":record slots are non-negative", bool((slots >= 0).all()))
            rmid, rhalf = 0.5 * (hi.max() + lo.max()), 0.5 * (hi.max() - lo.max())
            rep.add("%s:record" % what, np.array([v - rmid]), np.array([rhalf]))
            stored = float(got.max())
            rep.require("%s:record equals the stored maximum (%s)" % (what, kind),
                        v == stored if dt == DT_F32 else float(bf16_round(np.array([v], F32))[0]) == stored)
            if neg:
                rep.require(what + ":all-negative segment leaves its record at 0", v == 0.0 and stored == 0.0)
        else:
            assert recs[i] is None
    for bi, (ld, dt) in enumerate(k.buffers):
        sent = F32(SENT if dt == DT_F32 else SENT16)
        rep.require(what + ":columns outside the segments keep their sentinels",
                    bool((np.asarray(bufs[bi], F32)[~written[bi]] == sent).all()))
    return rep.check()


# ---- infer prepare ----------------------------------------------------------------------------------------------------------------
INFER_C = [1, 4, 255, 256, 257, 832, 1024]
INFER_MULTI = [1, 57, 64, 65, 130]
SQRTF_ULP = 1.0          # HIP math API, single precision table: sqrtf, 1 ulp
DIVIDE_ULP = 0.5         # correctly rounded (see infer_rstd_gate)


def infer_rstd_gate(mv, eps):
    """(reference, gate) of r = 1.0f / sqrtf(mv + eps).

    The library is built by csrc/Makefile (what build() runs) with `hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC`: no
    -ffast-math, no -fno-hip-fp32-correctly-rounded-divide-sqrt, no -fgpu-flush-denormals-to-zero
    (tests/test_bn_fwd_ref_cpu.py asserts this of the Makefile).  Under those flags the HIP math documentation gives sqrtf 1 ulp,
    and clang's default -fhip-fp32-correctly-rounded-divide-sqrt makes the fp32 division correctly rounded: half an ulp.  With
    the add's half ulp the gate is their sum, each ulp taken where it arises: the add's at a = mv + eps (it reaches r halved,
    d r / r = -d a / 2 a), sqrtf's at sqrt(a), the division's at r.  That is 0.5 + 1 + 0.5 = 2 ulps nominally, and at most
    0.25 + 2 + 0.5 where the binades of a, sqrt(a) and r sit worst."""
    a = np.asarray(mv, np.float64) + float(F32(eps))
    sq = np.sqrt(a)
    ref = 1.0 / sq
    rel = 0.5 * (0.5 * ulp32(a) / a) + SQRTF_ULP * ulp32(sq) / sq
    return ref, ref * rel + DIVIDE_ULP * ulp32(ref * (1.0 + rel))


def build_infer(C, seed=0):
    """beta, moving_mean, moving_var [C]: moving_var cycles through 0, values near 0 (rstd near 1 / sqrt(eps)), ordinary and
    large ones."""
    key = ("infer", C, seed)
    if key in _CACHE:
        return _CACHE[key]
    rng = np.random.RandomState(500 + 31 * seed + C)
    k = Case()
    k.C, k.eps = C, EPS
    k.beta = rng.normal(0, 0.3, size=C).astype(F32)
    k.mm = (rng.normal(size=C) * rng.choice([0.01, 1.0, 50.0], size=C)).astype(F32)
    special = np.array([0.0, 1e-12, 1e-7, 1e-4, 3e4, 1e6], F32)
    mv = rng.uniform(0.01, 4.0, size=C).astype(F32)
    sel = (np.arange(C) + seed) % 3 == 0
    mv[sel] = special[((np.arange(C) + seed) // 3 % len(special))[sel]]
    k.mv = mv
    k.r_ref, k.g_r = infer_rstd_gate(k.mv, k.eps)
    _CACHE[key] = k
    return k


def infer_multi_jobs(njobs):
    """The C of every job: the single form's values mixed, so a launch holds jobs below and above its widest."""
    return [INFER_C[(3 * j + j // 7) % len(INFER_C)] for j in range(njobs)]


def check_infer(k, rstd, shift, what="infer"):
    rep = Report()
    rstd, shift = np.asarray(rstd, F32), np.asarray(shift, F32)
    rep.add(what + ":rstd", rstd.astype(np.float64) - k.r_ref, k.g_r)
    t, g = shift_gate(k.beta, k.mm, rstd)
    rep.add(what + ":shift", shift.astype(np.float64) - t, g)
    return rep.check()
