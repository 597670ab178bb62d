"""fp64 checks of one conv launch that stay affordable at the batches the product runs (B = 256: 3.2 M output rows for the
stem).  Shared by tests/test_conv_layers_cpu.py (the checks themselves, with planted errors) and
tests/test_conv_layers_gpu.py (every conv plan the image engine builds).

A launch computes Z = A(X) for a linear map A: the SAME-padded convolution (forward), or its adjoint Conv2DBackpropInput
(dgrad).  Two checks together cover every output row:

  exact rows     every output row of a few images (0, one in the middle, N - 1: the ragged last tile) against the fp64
                 convolution of just those images, |got - ref| <= tol * max|ref|;
  projection     a random vector r over all M output rows: r^T Z against sum_taps (r^T X_tap) W_tap in fp64 (Freivalds).
                 A wrong, missing or duplicated tile anywhere in M moves r^T Z by ~ sqrt(rows of the tile) * |z|, rounding
                 by ~ ||r|| * rms(err); the bound is the per-element gate times ||r||_2.  Cost O(k^2 M Cin), no im2col.
"""
import numpy as np

from oracle import tf_semantics as S


def bf16_round(a):
    """round-to-nearest-even to bfloat16 (what v_cvt_pk_bf16_f32 does), as float64"""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32).astype(np.float64)


def bf16_ulp(a):
    """one unit in the last place of bfloat16 at |a| (8 significant bits; the smallest normal's step below it)"""
    m = np.maximum(np.abs(np.asarray(a, np.float64)), np.finfo(np.float32).tiny)
    return np.ldexp(1.0, np.frexp(m)[1] - 8)


def fp8_round(a, fmax, mant, emin):
    """saturating round-to-nearest-even to an OCP fp8 format (e4m3fn: 448, 3, -6; e5m2: 57344, 2, -14), as float64"""
    a = np.asarray(a, np.float64)
    m = np.minimum(np.abs(a), fmax)
    e = np.maximum(np.frexp(m)[1] - 1, emin)
    step = np.ldexp(1.0, e - mant)
    return np.sign(a) * np.rint(m / step) * step


def pow2_scale(amax, fmax):
    """the per-tensor power-of-two scale ds_conv_fp8 derives from a max|.| record"""
    if not amax > 0:
        return 1.0
    r = np.float32(fmax) / np.float32(amax)
    return float(2.0 ** (int(np.frexp(r)[1]) - 1))


E4M3 = (448.0, 3, -6)
E5M2 = (57344.0, 2, -14)


def tap_corr(a, b, k, stride, chunk=8):
    """G[i, j, ca, cb] = sum_{n, oh, ow} a_pad[n, oh*s + i, ow*s + j, ca] * b[n, oh, ow, cb] in fp64, with a zero-padded
    SAME for a k x k / stride-s window (= S.conv2d_same_bwd_filter(a, b, (k, k, Ca, Cb), s)) -- one image chunk and one tap
    at a time, so memory stays O(chunk * H * W * C)."""
    n, h, w, ca = a.shape
    oh, pt, pb = S.same_pad(h, k, stride)
    ow, pl, pr = S.same_pad(w, k, stride)
    assert b.shape[:3] == (n, oh, ow), (a.shape, b.shape)
    cb = b.shape[3]
    g = np.zeros((k, k, ca, cb))
    for n0 in range(0, n, chunk):
        ap = np.zeros((min(chunk, n - n0), h + pt + pb, w + pl + pr, ca))
        ap[:, pt:pt + h, pl:pl + w] = a[n0:n0 + chunk]
        bb = np.asarray(b[n0:n0 + chunk], np.float64)
        for i in range(k):
            for j in range(k):
                sl = ap[:, i:i + (oh - 1) * stride + 1:stride, j:j + (ow - 1) * stride + 1:stride]
                g[i, j] += np.tensordot(sl, bb, axes=([0, 1, 2], [0, 1, 2]))
    return g


class LinearConv:
    """Z = conv2d_same(X, w, s) ("fwd": X [N, H, W, Cin] -> Z [N, OH, OW, Cout]) or
    Z = Conv2DBackpropInput(X, w, s) ("dgrad": X = dz [N, OH, OW, Cout] -> Z = dx [N, H, W, Cin]), w HWIO [k, k, Cin, Cout]."""

    def __init__(self, role, w, stride, H, W):
        assert role in ("fwd", "dgrad")
        self.role, self.w, self.stride, self.H, self.W = role, np.asarray(w, np.float64), stride, H, W
        self.k = self.w.shape[0]

    def ref(self, x):
        """fp64 result for the images of x"""
        x = np.asarray(x, np.float64)
        if self.role == "fwd":
            return S.conv2d_same(x, self.w, self.stride)
        return S.conv2d_same_bwd_input(x, self.w, (x.shape[0], self.H, self.W, self.w.shape[2]), self.stride)

    def project(self, x, r):
        """r^T Z [Cout of Z] in fp64 without forming Z; r [N, rows of Z's grid]"""
        if self.role == "fwd":
            g = tap_corr(x, r[..., None], self.k, self.stride)[:, :, :, 0]           # [k, k, Cin]
            return np.tensordot(g, self.w, axes=([0, 1, 2], [0, 1, 2]))
        g = tap_corr(r[..., None], x, self.k, self.stride)[:, :, 0, :]               # [k, k, Cout]
        return np.tensordot(g, self.w, axes=([0, 1, 2], [0, 1, 3]))


def sample_images(n):
    """0, one in the middle, N - 1 (its last rows are the ragged last tile of every launch)"""
    return sorted({0, n // 2, n - 1})


class ConvCheck:
    """Checks of a launch's output `got` (float64 [N, ., ., C], the convolution part only: an accumulated operand already
    subtracted) against the fp64 map `op` applied to the operands `x` the kernel computed with (rounded / quantised
    already for the 16-bit families).  tol: the family's per-element gate as a fraction of max|ref|.  Every method returns
    worst error / gate (<= 1 passes) and records it in self.ratios."""

    def __init__(self, op, x, tol, rng, full_below=32):
        self.op, self.x, self.tol, self.rng = op, x, tol, rng
        self.n = x.shape[0]
        self.imgs = list(range(self.n)) if self.n <= full_below else sample_images(self.n)
        self.ref_imgs = op.ref(x[self.imgs])
        self.scale = max(float(np.abs(self.ref_imgs).max()), 1e-30)
        self.ratios = {}

    @property
    def gate(self):
        return self.tol * self.scale

    def rows(self, got, slack=None):
        """every row of the sampled images (all images when N <= full_below); slack: extra elementwise allowance, shaped like
        the sampled images' reference (a 16-bit store's ulp)"""
        g = np.asarray(got[self.imgs], np.float64)
        allow = self.gate if slack is None else self.gate + slack
        r = float((np.abs(g - self.ref_imgs) / allow).max())
        self.ratios["rows"] = r
        return r

    def projection(self, got, slack_rms=0.0):
        """r^T got against r^T ref over all rows, gate (tol * max|ref| + slack_rms) * ||r||_2 per column; slack_rms: the rms
        of an extra per-element error that is independent of r (the rounding of a 16-bit store)"""
        r = self.rng.standard_normal(got.shape[:3])
        lhs = np.tensordot(r, np.asarray(got, np.float64), axes=([0, 1, 2], [0, 1, 2])) if got.dtype == np.float64 else \
            _tensordot_chunked(r, got)
        rhs = self.op.project(self.x, r)
        q = float(np.abs(lhs - rhs).max() / ((self.gate + slack_rms) * np.linalg.norm(r)))
        self.ratios["proj"] = q
        return q

    def column_sums(self):
        """fp64 column sums of the reference over all rows (the projection with r = 1)"""
        return self.op.project(self.x, np.ones(self.n_grid()))

    def n_grid(self):
        if self.op.role == "fwd":
            oh, _, _ = S.same_pad(self.op.H, self.op.k, self.op.stride)
            ow, _, _ = S.same_pad(self.op.W, self.op.k, self.op.stride)
            return (self.n, oh, ow)
        return (self.n, self.op.H, self.op.W)

    def worst(self):
        return max(self.ratios.values()) if self.ratios else 0.0


def _tensordot_chunked(r, got, chunk=8):
    """r^T got for a float32 `got` without a float64 copy of the whole tensor"""
    acc = np.zeros(got.shape[3])
    for n0 in range(0, got.shape[0], chunk):
        acc += np.tensordot(r[n0:n0 + chunk], np.asarray(got[n0:n0 + chunk], np.float64), axes=([0, 1, 2], [0, 1, 2]))
    return acc


def sums_ratio(got, want, tol=2e-3):
    """column-sum check of the STATS / BNSUMS epilogues: max|got - want| / (tol * max|want|)"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.abs(got - want).max() / (tol * max(float(np.abs(want).max()), 1e-30)))
