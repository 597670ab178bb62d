"""Plain NumPy fp64 restatement of the two dense heads (JointHeadEngine, TextHeadEngine), the plan arithmetic of
ops.head_gemm_plan restated from its thresholds, the case lists of tests/test_head_dims_gpu.py and the comparison helpers of
the head / text-dimension / step-tail GPU tests.  Nothing here needs a GPU: tests/test_head_ref_cpu.py holds the heads against
torch.autograd in float64 and feeds every helper a planted error.

Joint:  dense = relu(im W_fc[:im] + tx W_fc[im:] + b_fc), logits = dense W_sm + b_sm     (im_text_rnn_model.py:95-105)
Text:   logits = h W_sm + b_sm                                                            (text_embedding.py:84-86)
Both take the mean softmax cross entropy over the batch."""
import numpy as np

U = 2.0 ** -24          # unit roundoff of fp32 (round to nearest)
REL = 2e-4              # the project's gate for the heads' GEMMs against fp64: REL * max|ref| per tensor


# ---- the heads ------------------------------------------------------------------------------------------------------------

def softmax_ce(logits, labels):
    """(mean cross entropy, d loss / d logits) in the dtype of `logits` (fp64 in)."""
    B = logits.shape[0]
    m = logits.max(1, keepdims=True)
    e = np.exp(logits - m)
    s = e.sum(1, keepdims=True)
    loss = float(np.mean(m[:, 0] + np.log(s[:, 0]) - logits[np.arange(B), labels]))
    p = e / s
    p[np.arange(B), labels] -= 1.0
    return loss, p / B


def joint_head(im, tx, W_fc, b_fc, W_sm, b_sm, labels, decisions=None):
    """decisions: a boolean [B, fc] -- which dense units are active -- to follow another forward pass's ReLU decisions
    (test_model_gpu._check_step does the same for the image tower); None: the reference's own."""
    n_im = im.shape[1]
    pre = im @ W_fc[:n_im] + tx @ W_fc[n_im:] + b_fc
    act = pre > 0 if decisions is None else np.asarray(decisions, bool)
    dense = np.where(act, pre, 0.0)
    logits = dense @ W_sm + b_sm
    loss, dlogits = softmax_ce(logits, labels)
    ddense = np.where(act, dlogits @ W_sm.T, 0.0)
    d_feat = ddense @ W_fc.T
    return dict(pre=pre, dense=dense, logits=logits, loss=loss, dlogits=dlogits, ddense=ddense,
                W_fc=np.concatenate([im.T @ ddense, tx.T @ ddense], 0), b_fc=ddense.sum(0),
                W_softmax=dense.T @ dlogits, b_softmax=dlogits.sum(0), d_im=d_feat[:, :n_im], d_tx=d_feat[:, n_im:])


def text_head(h, W_sm, b_sm, labels):
    logits = h @ W_sm + b_sm
    loss, dlogits = softmax_ce(logits, labels)
    return dict(logits=logits, loss=loss, dlogits=dlogits, W_softmax=h.T @ dlogits, b_softmax=dlogits.sum(0),
                d_tx=dlogits @ W_sm.T)


# ---- ops.head_gemm_plan, restated from its thresholds -----------------------------------------------------------------------

def plan_splits(M, K):
    """0: the plain plan; else the split count of the SplitGemm (M <= 512 and K >= 256: 8 from K = 512, else 4)."""
    return (8 if K >= 512 else 4) if (M <= 512 and K >= 256) else 0


def split_tiles(K, splits):
    """K-tiles (16 channels each) that every split of ds_conv_igemm's split-K owns: ceil(ceil(K / 16) / splits) each, the
    last ones what is left (0: an empty slice, its slab is all zeros)."""
    kt = -(-K // 16)
    kts = -(-kt // splits)
    return [max(0, min(kt, (s + 1) * kts) - s * kts) for s in range(splits)]


def split_ranges(K, splits):
    """[k0, k1) of every split (k1 == k0: empty)."""
    out, k0 = [], 0
    for n in split_tiles(K, splits):
        k1 = min(K, k0 + 16 * n)
        out.append((k0, k1))
        k0 = k1
    return out


def slice_form(K, splits):
    t = split_tiles(K, splits)
    return "empty" if t[-1] == 0 else ("ragged" if (len(set(t)) > 1 or K % 16) else "even")


def colsum_form(M):
    """ds_colsum: min(ceil(M / 64), 64) row splits; up to 8 of them (M <= 512) run as one launch."""
    return "one-launch" if min(-(-M // 64), 64) <= 8 else "two-stage"


def joint_forms(B, im, tx, fc, nc):
    """What JointHeadEngine reaches at these dims: per GEMM its split count (0 = plain), grouped / fused, and the set of
    form names the closing tests count."""
    plans = dict(fc_im=plan_splits(B, im), fc_tx=plan_splits(B, tx), sm=plan_splits(B, fc), sm_dgrad=plan_splits(B, nc),
                 im_dgrad=plan_splits(B, fc), tx_dgrad=plan_splits(B, fc))
    ks = dict(fc_im=im, fc_tx=tx, sm=fc, sm_dgrad=nc, im_dgrad=fc, tx_dgrad=fc)
    grouped = all(plans[k] for k in ("fc_im", "fc_tx", "im_dgrad", "tx_dgrad"))
    fused = bool(grouped and plans["sm"] and B <= 512 and nc <= 32)
    forms = {"grouped" if grouped else "ungrouped", "ce-fused" if fused else "ce-separate", "colsum-" + colsum_form(B)}
    for name, s in plans.items():
        forms.add("split%d" % s if s else "plain")
        if s:
            forms.add("slice-" + slice_form(ks[name], s))
    if fused and B > 256:
        forms.add("ce-fused-second-trip")
    return plans, grouped, fused, forms


def text_forms(B, H, nc):
    plans = dict(sm=plan_splits(B, H), sm_dgrad=plan_splits(B, nc))
    forms = {"colsum-" + colsum_form(B)}
    for name, s in plans.items():
        forms.add("split%d" % s if s else "plain")
        if s:
            forms.add("slice-" + slice_form(H if name == "sm" else nc, s))
    return plans, forms


ALL_FORMS = {"plain", "split4", "split8", "slice-even", "slice-ragged", "slice-empty", "grouped", "ungrouped", "ce-fused",
             "ce-separate", "ce-fused-second-trip", "colsum-one-launch", "colsum-two-stage"}

HEAD = (256, 512, 512, 15)          # the joint model's own head: im, tx, fc, nc
JOINT_CASES = (                      # (B, im, tx, fc, nc)
    [(B,) + HEAD for B in (1, 256, 257, 512, 513)] +
    [(33, 256, 255, 512, 15), (33, 256, 256, 512, 15), (33, 256, 512, 511, 15), (33,) + HEAD, (33, 256, 256, 256, 15),
     (33, 256, 512, 520, 15), (33, 256, 512, 560, 15), (33, 256, 648, 512, 15), (33, 260, 300, 512, 15)] +
    [(B, 256, 512, 512, nc) for nc in (2, 32, 33, 40) for B in (33, 257)] +
    # im * fc odd: W_fc's text half starts 4-byte aligned only (the scalar-load instantiations; the direct wgrad at B >= 512)
    [(33, 257, 512, 511, 15), (513, 257, 512, 511, 15)])
TEXT_CASES = [(B, H, nc) for H in (32, 255, 256, 520) for nc in (15, 33) for B in (1, 257, 513)]

# the head dims the suite ran before these tests (test_head_group_gpu, the model / multistep / clone / dp tests: rnn_size 32
# or 16 or 64 or 512 under the joint head 256 / 512 / 15, batches up to 130)
OLD_JOINT_CASES = ([(B,) + HEAD for B in (3, 8, 33, 130)] + [(B, 256, 32, 512, 15) for B in (2, 4, 8, 16, 32, 96)] +
                   [(8, 256, 64, 512, 15), (8, 256, 16, 512, 15), (4, 64, 32, 48, 15)])
OLD_TEXT_CASES = [(8, 16, 15), (5, 64, 15), (64, 512, 15), (8, 32, 15), (16, 32, 15)]


# ---- comparison helpers -----------------------------------------------------------------------------------------------------

class Worst:
    """The worst error / bound ratio a test has seen, printed at its end."""

    def __init__(self):
        self.ratio, self.what = 0.0, ""

    def take(self, ratio, what):
        if not ratio <= self.ratio:      # (NaN takes over)
            self.ratio, self.what = float(ratio), what

    def __str__(self):
        return "worst error / bound = %.3g (%s)" % (self.ratio, self.what)


def _f64(a):
    return np.asarray(a, np.float64)


def check_close(got, ref, what, rel=REL, worst=None):
    """max|got - ref| <= rel * max|ref| over the whole tensor (the kernel tests' gate); NaN fails."""
    got, ref = _f64(got).reshape(np.shape(ref)), _f64(ref)
    err = float(np.abs(got - ref).max()) if ref.size else 0.0
    bound = rel * max(float(np.abs(ref).max()), 1e-30)
    if worst is not None:
        worst.take(err / bound, what)
    assert err <= bound, "%s: max|err| %.3e above %.3e (%.1e of max|ref|)" % (what, err, bound, rel)
    return err / bound


def check_rows(got, ref, what, rel, floor=0.0, worst=None):
    """Every row against its own largest reference entry: max_c |got - ref| <= rel * max_c |ref| + floor."""
    got, ref = _f64(got).reshape(np.shape(ref)), _f64(ref)
    err = np.abs(got - ref).max(1)
    bound = rel * np.abs(ref).max(1) + floor
    ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    ratio = np.where(np.isnan(err), np.inf, ratio)
    r = int(np.argmax(ratio))
    if worst is not None:
        worst.take(float(ratio[r]), "%s row %d" % (what, r))
    assert ratio[r] <= 1.0, "%s: row %d (of %d rows failing) off by %.3e, bound %.3e" % (what, r, int((ratio > 1).sum()), err[r],
                                                                                    bound[r])
    return float(ratio[r])


def ce_row_floor(C, k):
    """Absolute rounding of one entry of dlogits = (softmax - onehot) k as softmax_ce_workgroup forms it, first order: the sum
    s of C exponentials in index order carries (C - 1) u, an exponential 2 u (expf) plus the rounding of its argument,
    p |z - m| u <= 0.4 u (x e^-x <= 1 / e), reciprocal and product 2 u -- (C + 3.4) u p in all, p <= 1 -- then the difference, k
    and the product with k one rounding each of a quantity <= 1: (C + 7) u k.  It matters only in rows whose label takes nearly
    all the probability: there every entry, the label's (p - 1) k included, is smaller than the rounding of p."""
    return (C + 7) * U * k


def check_bound(got, ref, bound, what, worst=None):
    """Elementwise |got - ref| <= bound (an array or a scalar, derived by the caller); NaN fails."""
    got, ref = _f64(got).reshape(np.shape(ref)), _f64(ref)
    err = np.abs(got - ref)
    bound = np.broadcast_to(_f64(bound), err.shape)
    bad = ~(err <= bound)
    ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    ratio = np.where(np.isnan(err), np.inf, ratio)
    i = int(np.argmax(ratio)) if ratio.size else 0
    if worst is not None and ratio.size:
        worst.take(float(ratio.reshape(-1)[i]), what)
    assert not bad.any(), "%s: %d of %d entries outside their bound, worst at flat index %d: |err| %.3e, bound %.3e" % (
        what, int(bad.sum()), bad.size, i, err.reshape(-1)[i], bound.reshape(-1)[i])
    return float(ratio.reshape(-1)[i]) if ratio.size else 0.0


def check_bits(got, ref, what):
    """The same fp32 bits (NaN patterns included; -0.0 differs from 0.0)."""
    a, b = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(ref, np.float32)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    diff = a.view(np.uint32) != b.view(np.uint32)
    assert not diff.any(), "%s: %d of %d entries differ in their bits, first at flat index %d (%r vs %r)" % (
        what, int(diff.sum()), diff.size, int(np.argmax(diff)), a.reshape(-1)[int(np.argmax(diff))],
        b.reshape(-1)[int(np.argmax(diff))])


# ---- ds_adam_tf -------------------------------------------------------------------------------------------------------------

def adam_model_f32(theta, g, m, v, n_wd, wd, grad_scale, lr_t, b1, b2, eps):
    """adam_tf_kernel's arithmetic in NumPy fp32, operation by operation (no contraction).  Returns (theta, m, v)."""
    f = np.float32
    theta, g, m, v = (np.asarray(a, f) for a in (theta, g, m, v))
    wd, grad_scale, lr_t, b1, b2, eps = f(wd), f(grad_scale), f(lr_t), f(b1), f(b2), f(eps)
    gi = g * grad_scale
    decayed = np.arange(theta.size) < n_wd
    gi = np.where(decayed, gi + wd * theta, gi).astype(f)
    mi = (b1 * m + (f(1) - b1) * gi).astype(f)
    vi = (b2 * v + (f(1) - b2) * gi * gi).astype(f)
    return (theta - lr_t * mi / (np.sqrt(vi) + eps)).astype(f), mi, vi


def adam_ref(theta, g, m, v, n_wd, wd, grad_scale, lr_t, b1, b2, eps):
    """One TF-Adam step in fp64 on fp32 inputs (the scalars are the fp32 values the kernel receives), with the first-order
    rounding bounds of adam_tf_kernel per element.  With G = |g gs| + wd |w| (the magnitude of the effective gradient's two
    terms), Mb = b1 |m| + (1 - b1) G, den = sqrt(v') + eps, Ub = lr_t Mb / den (the magnitude bound of the update):

      gi = g gs + wd w        two products and a sum: |d gi| <= 2 u G
      m' = b1 m + (1-b1) gi   1 - b1 is exact (Sterbenz); two products and a sum on top of d gi: |d m'| <= 4 u Mb
      v' = b2 v + (1-b2) gi^2 |d v'| <= (1-b2) 2 |gi| |d gi| + 3 u v' <= 4 u (1-b2) G^2 + 4 u v' <= 8 u (b2 v + (1-b2) G^2)
      den                     sqrt is 1/2-conditioned: (1-b2) |gi| 2 u G / sqrt(v') + 1.5 u sqrt(v'), sqrt's own rounding
                              (<= 2 u) and the sum's: |d den| <= 2 u sqrt(1-b2) G + 4.5 u den   (sqrt(v') >= sqrt(1-b2) |gi|)
      theta' = w - lr_t m' / den   product, quotient (<= 2 u) and the final rounding u |theta'|:
               |d theta'| <= u |theta'| + u Ub (4 + 4.5 + 3 + 2 sqrt(1-b2) G / den)

    The last term is the cancellation of g gs against wd w in the denominator; it is below 2 wherever they do not cancel.
    Returns (theta', m', v', bound_theta, bound_m, bound_v)."""
    d = np.float64
    w, g, m, v = (np.asarray(a, np.float32).astype(d) for a in (theta, g, m, v))
    wd, gs, lr_t, b1, b2, eps = (d(np.float32(a)) for a in (wd, grad_scale, lr_t, b1, b2, eps))
    decayed = np.arange(w.size) < n_wd
    gi = g * gs + np.where(decayed, wd * w, 0.0)
    G = np.abs(g * gs) + np.where(decayed, wd * np.abs(w), 0.0)
    m1 = b1 * m + (1 - b1) * gi
    v1 = b2 * v + (1 - b2) * gi * gi
    den = np.sqrt(v1) + eps
    t1 = w - lr_t * m1 / den
    Mb = b1 * np.abs(m) + (1 - b1) * G
    Ub = lr_t * Mb / den
    b_theta = U * np.abs(t1) + U * Ub * (11.5 + 2 * np.sqrt(1 - b2) * G / den)
    return t1, m1, v1, b_theta, 4 * U * Mb, 8 * U * (b2 * v + (1 - b2) * G * G)


def check_adam(got, before, g, n_wd, wd, grad_scale, lr_t, b1, b2, eps, what, worst=None):
    """got / before: (theta, m, v) fp32 arrays after / before ONE ds_adam_tf step.  Elements at or past n_wd whose gradient and
    moments are all zero must keep their bits (0 / (0 + eps) is 0); every other element is held to adam_ref's bound."""
    t0, m0, v0 = (np.asarray(a, np.float32) for a in before)
    g = np.asarray(g, np.float32)
    still = (np.arange(t0.size) >= n_wd) & (g == 0) & (m0 == 0) & (v0 == 0)
    t1, m1, v1, bt, bm, bv = adam_ref(t0, g, m0, v0, n_wd, wd, grad_scale, lr_t, b1, b2, eps)
    for name, a, b in (("theta", got[0], t0), ("m", got[1], m0), ("v", got[2], v0)):
        check_bits(np.asarray(a, np.float32)[still], b[still], "%s: %s of the undecayed zero-gradient entries" % (what, name))
    rest = ~still
    for name, a, r, b in (("theta", got[0], t1, bt), ("m", got[1], m1, bm), ("v", got[2], v1, bv)):
        check_bound(np.asarray(a, np.float32)[rest], r[rest], b[rest], "%s: %s" % (what, name), worst)


def adam_inputs(n, n_wd, seed, stretch=16):
    """theta, three gradients: N(0, 1) weights, 1e-3 N(0, 1) gradients, and `stretch` elements either side of n_wd with weights
    of magnitude 0.5 .. 1.5 and zero gradients at every step: undecayed they must not move at all, decayed they move by
    about lr per step (wd |w| >> eps), so a boundary off by one is an lr-sized error."""
    rng = np.random.RandomState(seed)
    w = rng.normal(size=n).astype(np.float32)
    lo, hi = max(0, n_wd - stretch), min(n, n_wd + stretch)
    w[lo:hi] = (rng.uniform(0.5, 1.5, size=hi - lo) * rng.choice([-1.0, 1.0], size=hi - lo)).astype(np.float32)
    gs = []
    for _ in range(3):
        g = (rng.normal(size=n) * 1e-3).astype(np.float32)
        g[lo:hi] = 0.0
        gs.append(g)
    return w, gs
