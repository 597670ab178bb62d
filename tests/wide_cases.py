"""The instantiations and loaders of gemm_wide_kernel (the wide 1x1 kernel of conv_igemm.hip), shared by test_wide_cases_cpu.py
(the builders' own assertions, the comparison helpers against planted errors, the host launch choice read back through
ds_debug_conv_igemm_launch without a device) and test_wide_gpu.py (the kernel against the fp64 reference).  numpy only.

A case is one launch: a variant (which loader and which side of the weights), the pinned column blocks per wave, a shape and a
mode (which epilogue).  `build(case)` makes EXACT operands -- small integers and dyadic per-channel values -- and asserts, in
fp64, the condition under which equality with the fp64 reference is a fair demand of ANY fp32 evaluation order, fused or not:
every term of every output element and of every statistics partial is an integer multiple of one power-of-two quantum, and the
sum of the terms' absolute values stays below 2^24 quanta, so no partial sum of them is ever rounded.  `real_case(variant, nb)` names
one launch per instantiation whose operands `build` draws from normal distributions, so that exactness cannot hide a precision loss.

The reference is the documented operation in fp64: relu(x r + s) @ w, bn_bwd_ref.reference(...).dz @ w^T,
S.max_pool(...) @ w with S.max_pool_argmax, prev + ... under DS_EPI_ACCUM, relu(z scale + shift) under DS_EPI_BN_RELU, and the
DS_EPI_STATS / DS_EPI_BNSUMS sums per 128-row partial."""
import functools
import zlib

import numpy as np

import bn_bwd_ref as BR
from oracle import tf_semantics as S

EPI_ACCUM, EPI_STATS, EPI_BNSUMS, EPI_BN_RELU = 4, 8, 32, 64
LIMIT = 2.0 ** 24          # quanta
X_PAD = 7.0                # the row padding of x (finite: the kernel may read it against zero weights)
Y_PAD = 3.0                # the row padding of the BatchNorm-sums activation (positive: a column past Cout would switch on)
GUARD = 5.0                # z: guard rows in front and behind, columns right of Cout
GUARD_ROWS = 3
CANARY = -77.0             # behind the statistics partials
CANARY_LEN = 64
WINNER_FILL = 77           # the winners' buffer before the launch, and its canary behind (a winner is 0 .. 8)

# variant -> (n-contiguous weights, bnb, pool, DS_EPI_BN_RELU), the pins it is instantiated for, its modes
VARIANTS = {
    "fwd": ((1, 0, 0, 0), range(1, 9), ("plain", "stats", "stats0")),
    "dgrad": ((0, 0, 0, 0), range(1, 9), ("plain", "accum", "accum_bnsums", "bnsums_rstd")),
    "norm": ((1, 0, 0, 0), range(1, 9), ("stats",)),
    "bnb": ((0, 1, 0, 0), range(1, 3), ("plain", "accum_bnsums", "accum_bnsums_rstd")),
    "pool": ((1, 0, 1, 0), range(1, 5), ("stats",)),
    "poolnorm": ((1, 0, 1, 0), range(1, 5), ("stats",)),
    "bnr": ((1, 0, 0, 1), range(1, 9), ("bnr",)),
    "poolbnr": ((1, 0, 1, 1), range(1, 5), ("bnr",)),
}
VARIANT_NB = [(v, nb) for v in VARIANTS for nb in VARIANTS[v][1]]


def instantiation(variant, nb):
    """(NB, n-contiguous weights, BNB, POOL, BNR): the template arguments kernel_of() picks."""
    return (nb,) + VARIANTS[variant][0]


ALL_INSTANTIATIONS = frozenset(instantiation(v, nb) for v, nb in VARIANT_NB)

# POOL: the maps of test_pool_on_load_gpu.py (blocks that straddle two images, surplus waves, halo rows from memory and from
# the tile, a width that does not divide 32) and the reduction lengths (one K step and several)
POOL_MAPS = ((3, 14, 14, 48), (5, 7, 7, 16), (2, 28, 28, 32), (3, 9, 11, 48))
POOL_COUT = {1: (32,), 2: (40,), 3: (96,), 4: (100, 128)}
BNB_ENDS = {32: (32,), 40: (16, 32, 40), 296: (160, 296), 1024: (512, 1008, 1024)}


class Case:
    def __init__(self, variant, nb, mode, M, K, Cout, hw=None, real=False):
        self.variant, self.nb, self.mode, self.M, self.K, self.Cout, self.hw, self.real = variant, nb, mode, M, K, Cout, hw, real
        self.key = (variant, nb, mode, M, K, Cout, hw, real)
        self.n_contig, self.bnb, self.pool, self.bnr = (bool(f) for f in VARIANTS[variant][0])
        self.norm = variant in ("norm", "poolnorm") or (variant == "poolbnr" and hw is not None and hw[1] in (7, 9))
        self.ldx = K + 8
        self.ldz = Cout + 4
        self.ldmask = Cout + 8
        self.flags = {"plain": 0, "stats": EPI_STATS, "stats0": EPI_STATS, "accum": EPI_ACCUM,
                      "accum_bnsums": EPI_ACCUM | EPI_BNSUMS, "accum_bnsums_rstd": EPI_ACCUM | EPI_BNSUMS,
                      "bnsums_rstd": EPI_BNSUMS, "bnr": EPI_BN_RELU}[mode]
        self.ends = BNB_ENDS[K] if self.bnb else None
        # a launch that is not pooled writes one partial per 128-row tile; a pooled one, one per four 32-pixel blocks of whole
        # image rows (pool3_blocks)
        if self.pool:
            n, h, w = hw
            rpb = 32 // w
            self.partials = -(-n * (-(-h // rpb)) // 4)
        else:
            self.partials = -(-M // 128)
        self.col_tiles = -(-Cout // (32 * nb))

    def __repr__(self):
        s = "%s-nb%d-%s-" % (self.variant, self.nb, self.mode)
        s += ("%dx%dx%d" % self.hw if self.hw else "M%d" % self.M) + "-K%d-N%d" % (self.K, self.Cout)
        return s + ("-real" if self.real else "")

    def __hash__(self):
        return hash(self.key)

    def __eq__(self, other):
        return self.key == other.key

    def desc_fields(self):
        """The ds_conv_desc of the launch (the on-load pointers and `partials` are the caller's)."""
        n, h, w = self.hw if self.pool else (self.M, 1, 1)
        f = dict(N=n, H=h, W=w, Cin=self.K, ldx=self.ldx, KH=1, KW=1, stride=1, pad_t=0, pad_l=0, OH=h, OW=w, Cout=self.Cout,
                 ldz=self.ldz, w_tap_stride=self.K * self.Cout, flip=0, fold_cin=0, flags=self.flags, ldmask=0, splits=1, dtype=0)
        if self.n_contig:
            f.update(w_n_stride=1, w_k_stride=self.Cout)          # HWIO [K][Cout]
        else:
            f.update(w_n_stride=self.K, w_k_stride=1)             # a dgrad reads [Cout][K] in place
        if self.flags & EPI_BNSUMS:
            f["ldmask"] = self.ldmask
        return f


def shapes(nb):
    """(M, K, Cout) of the launches that are not pooled, per pin.  Rows: 165 (row tile 1 has wave 0 full, wave 1 with five rows,
    waves 2 and 3 empty; two row tiles on a grid rounded up to 8 workgroups, so some own no tile), 37, 256.  Reduction: 32, 40 (a
    K tail of 8 in the last 16-channel step), 296, and 1024 (the limit of the per-channel LDS tables) at NB 2 and 8.  Columns:
    32 NB - 28 (one column tile whose last block has 4 real columns) and 32 NB + 4 (a second, nearly empty column tile)."""
    c1, c2 = 32 * nb - 28, 32 * nb + 4
    t = [(165, 40, c1), (165, 296, c2), (37, 32, c2), (256, 40, c2), (37, 296, c1), (256, 32, c1)]
    if nb in (2, 8):
        t.append((165, 1024, c2))
    return t


@functools.lru_cache(maxsize=None)
def cases(variant, nb):
    modes = VARIANTS[variant][2]
    if variant in ("pool", "poolnorm", "poolbnr"):
        return tuple(Case(variant, nb, m, n * h * w, k, co, hw=(n, h, w)) for (n, h, w, k) in POOL_MAPS for co in POOL_COUT[nb]
                     for m in modes)
    return tuple(Case(variant, nb, m, M, K, co) for (M, K, co) in shapes(nb) for m in modes)


@functools.lru_cache(maxsize=None)
def real_case(variant, nb):
    """The one real-valued launch of an instantiation: two row tiles with a ragged second one, a K tail, two column tiles; the
    epilogue with the most in it."""
    mode = {"fwd": "stats", "dgrad": "accum_bnsums", "norm": "stats", "bnb": "accum_bnsums", "pool": "stats", "poolnorm": "stats",
            "bnr": "bnr", "poolbnr": "bnr"}[variant]
    if variant in ("pool", "poolnorm", "poolbnr"):
        n, h, w, k = POOL_MAPS[0]
        return Case(variant, nb, mode, n * h * w, k, POOL_COUT[nb][-1], hw=(n, h, w), real=True)
    return Case(variant, nb, mode, 165, 40, 32 * nb + 4, real=True)


def all_cases():
    return [c for v, nb in VARIANT_NB for c in cases(v, nb)]


# ---- exactness ------------------------------------------------------------------------------------------------------------------
def is_multiple(a, q):
    a = np.asarray(a, np.float64) / q
    return bool(np.array_equal(a, np.round(a)))


def quantum_of(a):
    """The largest power of two (at most 1) that divides every element of a."""
    q = 1.0
    while not is_multiple(a, q):
        q /= 2
        assert q >= 2.0 ** -12, "not dyadic"
    return q


def assert_exact_products(A, W):
    """A [M, K] @ W [K, N]: every product is a multiple of q = q(A) q(W) and every output element's sum of |products| is below
    2^24 q.  Returns q."""
    q = quantum_of(A) * quantum_of(W)
    total = (np.abs(A) @ np.abs(W)).max() / q
    assert total < LIMIT, "sum of |products| = %.0f quanta" % total
    return q


def assert_exact_sum(terms, q, what):
    """A sum over the rows of `terms` [rows, N] (one statistics partial, or z = acc + prev as a two-term sum)."""
    assert is_multiple(terms, q), what
    total = np.abs(terms).sum(0).max() / q if terms.size else 0.0
    assert total < LIMIT, "%s: sum of |terms| = %.0f quanta" % (what, total)


def pooled_partial_rows(c):
    """The pixels of each statistics partial of a pooled launch: a wave takes a block of 32 // W whole image rows of one image,
    a workgroup four consecutive blocks (which may straddle two images)."""
    n, h, w = c.hw
    rpb = 32 // w
    blocks = [np.arange((i * h + r0) * w, (i * h + min(h, r0 + rpb)) * w) for i in range(n) for r0 in range(0, h, rpb)]
    rows = [np.concatenate(blocks[j:j + 4]) for j in range(0, len(blocks), 4)]
    assert len(rows) == c.partials and sum(len(r) for r in rows) == c.M
    return rows


class Problem:
    pass


def _weights(c, rng):
    """The weight tensor as stored, and as the [K, Cout] matrix of the reference."""
    if c.real:
        w = (rng.normal(size=(c.K, c.Cout)) * 0.1).astype(np.float32)
    else:
        w = rng.randint(-1, 2, size=(c.K, c.Cout)) if c.K >= 1024 else rng.randint(-2, 3, size=(c.K, c.Cout))
        w = w.astype(np.float32)
    stored = np.ascontiguousarray(w if c.n_contig else w.T)
    return stored, w.astype(np.float64)


def _pad(a, ld, value):
    out = np.full((a.shape[0], ld), value, np.float32)
    out[:, :a.shape[1]] = a
    return out


def _norm_operands(c, rng, x):
    """rstd in {0.5, 1, 2}, shift a multiple of 0.25; a leading quarter of the channels carries (1, 0) on non-negative x (a
    Branch_0 slice of activations); every channel holds elements with x rstd + shift < 0, == 0 and > 0."""
    K = c.K
    if c.real:
        r = (np.abs(rng.normal(size=K)) + 0.5).astype(np.float32)
        s = (rng.normal(size=K) * 0.3).astype(np.float32)
    else:
        r = rng.choice([0.5, 1.0, 2.0], size=K).astype(np.float32)
        s = (rng.randint(-4, 5, size=K) * 0.25).astype(np.float32)
    r[:K // 4], s[:K // 4] = 1.0, 0.0
    x[..., :K // 4] = np.abs(x[..., :K // 4])
    if not c.real:
        flat = x.reshape(-1, K)
        rows = rng.permutation(flat.shape[0])[:3] if flat.shape[0] >= 3 else None
        if rows is not None:
            # three rows hold, in the channels that are normalised, a negative, a zero and a positive pre-activation
            for ch in range(K // 4, K):
                zero = -s[ch] / r[ch]                       # (|zero| <= 2: a multiple of 0.125; x is rounded to the integer grid ...)
                zi = np.round(zero)
                if zi * r[ch] + s[ch] != 0:                 # (... and the shift moved with it)
                    s[ch] = -zi * r[ch]
                flat[rows[0], ch], flat[rows[1], ch], flat[rows[2], ch] = zi - 1, zi, zi + 1
            t = flat[:, K // 4:] * r[K // 4:].astype(np.float64) + s[K // 4:]
            assert ((t < 0).any(0) & (t == 0).any(0) & (t > 0).any(0)).all()
    return r, s


def _build(c):
    rng = np.random.RandomState(zlib.crc32(repr(c.key[:-1]).encode()) & 0x7FFFFFFF)
    p = Problem()
    p.case = c
    M, K, N = c.M, c.K, c.Cout
    p.w, W = _weights(c, rng)
    p.rstd = p.shift = p.bnb = p.winners = None
    # ---- the A operand: what the loader makes of x
    if c.bnb:
        b = BR.build_real(M, K, 40 + c.nb) if c.real else BR.build_exact(M, K, 40 + c.nb)
        p.bnb = b
        p.x = _pad(b.z, c.ldx, X_PAD)
        p.dy_parts, c0 = [], 0
        for i, c1 in enumerate(c.ends):       # each range in its own buffer with its own row stride
            p.dy_parts.append((c0, c1, _pad(b.dy[:, c0:c1], (c1 - c0 + 3) // 4 * 4 + (4, 12, 24)[i], 9.0)))
            c0 = c1
        A = BR.reference(b.z, b.dy, b.mean, b.rstd, b.shift, b.coef).dz
    else:
        shape = (c.hw + (K,)) if c.pool else (M, K)
        if c.real:
            x = np.round(rng.normal(size=shape) * 3) / 3 if c.pool else rng.normal(size=shape)      # (pool: ties inside the windows)
            x = x.astype(np.float32).astype(np.float64)
        else:
            x = (rng.randint(-1, 2, size=shape) if K >= 1024 else rng.randint(-2, 3, size=shape)).astype(np.float64)
        if c.norm:
            p.rstd, p.shift = _norm_operands(c, rng, x)
        p.x = _pad(x.reshape(M, K), c.ldx, X_PAD)
        A = x
        if c.pool:
            p.winners = S.max_pool_argmax(x, 3, 1, "SAME").reshape(M, K)
            A = S.max_pool(x, 3, 1, "SAME")
        if c.norm:
            # (the pooled maximum is taken over the raw values and normalised once: rstd > 0)
            A = np.maximum(A * p.rstd.astype(np.float64) + p.shift.astype(np.float64), 0.0)
        A = A.reshape(M, K)
    p.A = A
    acc = A @ W
    q = None if c.real else assert_exact_products(A, W)
    p.quantum = q
    # ---- the epilogue
    p.prev = p.mask = p.mask_rstd = p.mask_shift = p.pivot = p.scale = p.bn_shift = p.stats = p.stat_terms = None
    z = acc
    if c.flags & EPI_ACCUM:
        p.prev = (rng.normal(size=(M, N)) if c.real else rng.randint(-8, 9, size=(M, N))).astype(np.float32)
        z = acc + p.prev
        if not c.real:
            assert is_multiple(p.prev, q) and (np.abs(acc) + np.abs(p.prev)).max() / q < LIMIT
    if c.flags & EPI_BN_RELU:
        # dyadic scale and shift; one column clamped everywhere
        if c.real:
            p.scale = (np.abs(rng.normal(size=N)) + 0.5).astype(np.float32)
            p.bn_shift = (rng.normal(size=N) * 0.3).astype(np.float32)
        else:
            p.scale = rng.choice([0.5, 1.0, 2.0], size=N).astype(np.float32)
            p.bn_shift = (rng.randint(-8, 9, size=N) * 0.25).astype(np.float32)
            p.bn_shift[N // 2] = -np.ceil(np.abs(acc[:, N // 2]).max() * 2 + 1)
        z = np.maximum(acc * p.scale.astype(np.float64) + p.bn_shift.astype(np.float64), 0.0)
        if not c.real:
            assert (z[:, N // 2] == 0).all() and (z > 0).any()
            assert ((np.abs(acc) * 2 + np.abs(p.bn_shift)).max() / (q * 0.25)) < LIMIT
    p.z = z
    rows_of = [slice(i * 128, min(M, (i + 1) * 128)) for i in range(c.partials)] if not c.pool else [slice(0, M)]
    exact_rows = rows_of if not c.pool else pooled_partial_rows(c)
    if c.flags & EPI_STATS:
        if c.mode == "stats":
            # an integer pivot, nonzero in every column: a phantom row contributes -pivot visibly
            p.pivot = (rng.normal(size=N) * 0.1).astype(np.float32) if c.real else \
                (rng.randint(1, 4, size=N) * rng.choice([-1, 1], size=N)).astype(np.float32)
        pv = p.pivot.astype(np.float64) if p.pivot is not None else np.zeros(N)
        p.stat_terms = (z - pv, (z - pv) ** 2)
    if c.flags & EPI_BNSUMS:
        if c.mode.endswith("_rstd"):
            # a consumer's z with dyadic rstd / shift, positive shifts among them: a row past M (read as 0) must not switch on
            # (behind the BatchNorm backward on load the gradient is on a 2^-6 grid: a narrower consumer keeps g y below 2^24)
            zc = rng.normal(size=(M, N)) if c.real else (rng.randint(-1, 2, size=(M, N)) if c.bnb else rng.randint(-2, 3, size=(M, N)))
            p.mask = _pad(zc.astype(np.float32), c.ldmask, Y_PAD)
            if c.real:
                p.mask_rstd = (np.abs(rng.normal(size=N)) + 0.5).astype(np.float32)
                p.mask_shift = (rng.normal(size=N) * 0.3).astype(np.float32)
            else:
                p.mask_rstd = rng.choice([0.5, 1.0, 2.0], size=N).astype(np.float32)
                p.mask_shift = (rng.randint(-3, 4, size=N) * 0.25).astype(np.float32)
                p.mask_shift[::3] = 0.75
            y = np.maximum(p.mask[:, :N].astype(np.float64) * p.mask_rstd + p.mask_shift, 0.0)
        else:
            # y on a 0.25 grid with about 30 % zeros
            y = np.abs(rng.normal(size=(M, N))) if c.real else rng.randint(1, 5, size=(M, N)) * 0.25
            y = (y * (rng.uniform(size=(M, N)) < 0.7)).astype(np.float32)
            p.mask = _pad(y, c.ldmask, Y_PAD)
            y = y.astype(np.float64)
        p.y = y
        g = np.where(y > 0, z, 0.0)
        p.stat_terms = (g, g * y)
    if p.stat_terms is not None:
        p.stats = np.stack([np.stack([t[r].sum(0) for r in rows_of], axis=1) for t in p.stat_terms])      # [2][Cout][P or 1]
        if not c.real:
            qs = (q, q * q) if c.flags & EPI_STATS else (q, q * quantum_of(p.y))
            for t, qt, name in zip(p.stat_terms, qs, ("sum", "sum of squares / of g y")):
                for r in exact_rows:
                    assert_exact_sum(t[r], qt, name)
    for v in vars(p).values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def build(case):
    """Cached: a reference is computed once and shared; callers do not modify what they get (the arrays are read-only)."""
    return _build(case)


# ---- comparison helpers (numpy arrays as copied back from the device) -------------------------------------------------------------
def z_buffer(p, fill=None):
    """The output buffer before the launch: GUARD_ROWS guard rows, M rows of ldz floats, GUARD_ROWS guard rows, everything GUARD
    except -- under DS_EPI_ACCUM -- the previous values."""
    c = p.case
    buf = np.full((2 * GUARD_ROWS + c.M, c.ldz), GUARD, np.float32)
    if p.prev is not None:
        buf[GUARD_ROWS:GUARD_ROWS + c.M, :c.Cout] = p.prev
    elif fill is not None:
        buf[GUARD_ROWS:GUARD_ROWS + c.M, :c.Cout] = fill
    return buf


def check_z(buf, p, ref=None):
    """Every element equal to the fp64 reference; the guard rows and the columns right of Cout untouched."""
    c = p.case
    ref = p.z if ref is None else ref
    got = buf[GUARD_ROWS:GUARD_ROWS + c.M, :c.Cout].astype(np.float64)
    bad = np.argwhere(got != ref)
    assert bad.size == 0, "%r: z differs at %d of %d elements, first (row %d, column %d): %r against %r" % (
        c, len(bad), got.size, bad[0][0], bad[0][1], got[tuple(bad[0])], ref[tuple(bad[0])])
    assert np.array_equal(got, ref)
    outside = buf.copy()
    outside[GUARD_ROWS:GUARD_ROWS + c.M, :c.Cout] = GUARD
    assert np.array_equal(outside, np.full_like(outside, GUARD)), "%r: a guard of z was overwritten" % (c,)


def stats_buffer(p):
    c = p.case
    buf = np.full(2 * c.Cout * c.partials + CANARY_LEN, np.nan, np.float32)
    buf[-CANARY_LEN:] = CANARY
    return buf


def check_stats(buf, p, ref=None):
    """Per partial for a launch that is not pooled, per column total for a pooled one (whose partials group other rows); every
    partial written (the buffer started as NaN), the canary behind intact."""
    c = p.case
    ref = p.stats if ref is None else ref
    n = 2 * c.Cout * c.partials
    got = buf[:n].astype(np.float64).reshape(2, c.Cout, c.partials)
    assert not np.isnan(got).any(), "%r: %d statistics partials were not written" % (c, int(np.isnan(got).sum()))
    if c.pool:
        got = got.sum(2, keepdims=True)
    bad = np.argwhere(got != ref)
    assert bad.size == 0, "%r: statistics differ at %d places, first [%d][column %d][partial %d]: %r against %r" % (
        c, len(bad), bad[0][0], bad[0][1], bad[0][2], got[tuple(bad[0])], ref[tuple(bad[0])])
    assert np.array_equal(got, ref)
    assert np.array_equal(buf[n:], np.full(CANARY_LEN, CANARY, np.float32)), "%r: the canary behind the statistics" % (c,)


def winners_buffer(p):
    return np.full(p.case.M * p.case.K + CANARY_LEN, WINNER_FILL, np.uint8)


def check_winners(buf, p):
    c = p.case
    n = c.M * c.K
    got = buf[:n].reshape(c.M, c.K)
    assert not (got == WINNER_FILL).any(), "%r: %d winner bytes were not written" % (c, int((got == WINNER_FILL).sum()))
    assert np.array_equal(got, p.winners), "%r: winners differ at %d of %d positions" % (c, int((got != p.winners).sum()), n)
    assert (buf[n:] == WINNER_FILL).all(), "%r: the canary behind the winners" % (c,)


# ---- the real-valued gates ---------------------------------------------------------------------------------------------------------
Z_TOL = 2e-4               # test_kernels_gpu.py's own gate: 2e-4 max|ref|


def real_stats_check(buf, p, z_stored):
    """The sums against fp64 sums over the kernel's OWN stored z: (128 + 4) 2^-24 sum|term| per partial (128 rows per partial:
    bn_bwd_ref.sums_tol with n = 128); pooled launches per column total, the bound summed likewise.  Returns the worst
    error / bound."""
    c = p.case
    z = z_stored.astype(np.float64)
    if c.flags & EPI_STATS:
        pv = p.pivot.astype(np.float64) if p.pivot is not None else 0.0
        terms = (z - pv, (z - pv) ** 2)
    else:
        g = np.where(p.y > 0, z, 0.0)
        terms = (g, g * p.y)
    n = 2 * c.Cout * c.partials
    got = buf[:n].astype(np.float64).reshape(2, c.Cout, c.partials)
    assert np.array_equal(buf[n:], np.full(CANARY_LEN, CANARY, np.float32))
    rows_of = [slice(i * 128, min(c.M, (i + 1) * 128)) for i in range(c.partials)] if not c.pool else [slice(0, c.M)]
    if c.pool:
        got = got.sum(2, keepdims=True)
    worst = 0.0
    for k, t in enumerate(terms):
        for i, r in enumerate(rows_of):
            tol = BR.sums_tol(128, np.abs(t[r]).sum(0))
            err = np.abs(got[k, :, i] - t[r].sum(0))
            assert (err <= tol).all(), "%r: sums[%d] partial %d off by %.3e against %.3e" % (c, k, i, err.max(), tol[err.argmax()])
            worst = max(worst, float((err / np.maximum(tol, 1e-300)).max()))
    return worst


# ---- the descriptor and the host launch choice ---------------------------------------------------------------------------------
def make_desc(case):
    """ds_conv_desc (ctypes) of the case, without the on-load pointers."""
    from tumblr_emotions_amd import _lib
    d = _lib.ConvDesc()
    for k, v in case.desc_fields().items():
        setattr(d, k, v)
    return d


def launch_of(lib, d):
    """ds_debug_conv_igemm_launch (the tuning library): (wide NB or 0, n-contiguous weights, bnb, pool, DS_EPI_BN_RELU, mt, nt,
    LDS-DMA kernel, workgroups launched, statistics partials)."""
    import ctypes as C
    out = (C.c_int * 10)()
    assert lib.ds_debug_conv_igemm_launch(C.byref(d), out) == 0, lib.ds_last_error()
    return tuple(out)


class pinned:
    """with pinned(lib, nb): the wide kernel wherever the shape allows, `nb` column blocks per wave; back at the defaults after."""

    def __init__(self, lib, nb):
        self.lib, self.nb = lib, nb

    def __enter__(self):
        assert self.lib.ds_debug_conv_set_wide(2) == 0 and self.lib.ds_debug_conv_set_wide_nb(self.nb) == 0

    def __exit__(self, *exc):
        assert self.lib.ds_debug_conv_set_wide(1) == 0 and self.lib.ds_debug_conv_set_wide_nb(0) == 0
        return False


def expected_launch(case):
    """What the launch query must answer for the case under its pin: the instantiation, one workgroup per (row tile, column tile)
    on a 1-D grid rounded up to 8, one statistics partial per row tile."""
    col_tiles = 1 if case.pool else case.col_tiles
    wgs = -(-case.partials * col_tiles // 8) * 8
    return instantiation(case.variant, case.nb), wgs, case.partials
