"""fp64 restatement of slim.losses.softmax_cross_entropy(logits, onehot, weights, label_smoothing) as the training step uses
it, its torch form for the oracle model, and the comparison helpers of tests/test_loss_options_gpu.py.
Nothing here needs a GPU: tests/test_loss_options_cpu.py holds the gradient against torch.autograd in float64 and feeds every
helper a planted error.  [TF-sem]: TF 1.x restated, TensorFlow is not in the reference tree, parity unpinned.

For B rows, C classes, smoothing e and class weights cw (None: all ones):
    q_bc = onehot(y_b)_c (1 - e) + e / C            (TF: onehot * smooth_positives + smooth_negatives; a label outside [0, C)
                                                     has an all-zero one-hot row)
    l_b  = sum_c q_bc (lse_b - z_bc)                 lse_b = m_b + log sum_c exp(z_bc - m_b)
    w_b  = cw[y_b]                                   (1 for a label outside [0, C))
    P    = #{b : w_b != 0}                           (compute_weighted_loss, SUM_BY_NONZERO_WEIGHTS)
    loss = sum_b w_b l_b / P                         (0 when P == 0; NaN when some label is outside [0, C))
    dlogits_bc = (softmax_bc - q_bc) w_b grad_scale / P      (all 0 when P == 0)"""
import numpy as np
import torch

import head_ref as HR

U = HR.U
NAN = float("nan")


def terms(logits, labels, label_smoothing=0.0, class_weights=None):
    """(softmax p [B, C], q [B, C], w [B], P, l [B], in-range mask [B]) in float64."""
    z = np.asarray(logits, np.float64)
    y = np.asarray(labels).astype(np.int64)
    B, C = z.shape
    ok = (y >= 0) & (y < C)
    onehot = np.zeros_like(z)
    onehot[np.arange(B)[ok], y[ok]] = 1.0
    q = onehot * (1.0 - label_smoothing) + label_smoothing / C
    m = z.max(1, keepdims=True)
    e = np.exp(z - m)
    s = e.sum(1, keepdims=True)
    lse = m + np.log(s)
    l = (q * (lse - z)).sum(1)
    w = np.ones(B)
    if class_weights is not None:
        cw = np.asarray(class_weights, np.float64)
        assert cw.shape == (C,)
        w[ok] = cw[y[ok]]
    return e / s, q, w, int((w != 0).sum()), l, ok


def softmax_ce(logits, labels, label_smoothing=0.0, class_weights=None, grad_scale=1.0):
    """(loss, d loss / d logits * grad_scale) in float64."""
    p, q, w, P, l, ok = terms(logits, labels, label_smoothing, class_weights)
    if P == 0:
        return 0.0, np.zeros_like(p)
    live = w != 0
    loss = float((w[live] * l[live]).sum() / P) if ok.all() else NAN
    return loss, (p - q) * (w * (grad_scale / P))[:, None]


def torch_ce(logits, labels, label_smoothing=0.0, class_weights=None):
    """The same loss written out on torch tensors (differentiable; labels inside [0, C)): what the oracle model's loss()
    returns in place of F.cross_entropy.  Not F.cross_entropy(weight=): that divides by sum w, not by the count of non-zero w."""
    labels = torch.as_tensor(labels).long()
    B, C = logits.shape
    q = torch.nn.functional.one_hot(labels, C).to(logits.dtype) * (1.0 - label_smoothing) + label_smoothing / C
    lse = torch.logsumexp(logits, dim=1, keepdim=True)
    l = (q * (lse - logits)).sum(1)
    if class_weights is None:
        w = torch.ones(B, dtype=logits.dtype)
    else:
        w = torch.as_tensor(np.asarray(class_weights, np.float64)).to(logits.dtype)[labels]
    P = int((w != 0).sum())
    if P == 0:
        return (l * 0.0).sum()
    return (w * l).sum() / P


# ---- comparison helpers -----------------------------------------------------------------------------------------------------

def row_floor(C, w, k):
    """Absolute rounding of one entry of dlogits = (softmax - q) (w k), k = grad_scale / P, as softmax_ce_workgroup<true> forms
    it, first order, derived the way HR.ce_row_floor is.  softmax p carries (C + 3.4) u p (there).  q = (label ? 1 - e : 0) +
    e / C: beside the label e / C alone, one rounding u q; at the label the roundings of 1 - e, of e / C and of their sum, at
    most 2 u q.  Then the difference p - q, the quotient k, the product w k and the last product, one rounding each of a
    quantity |p - q| <= 1: in units of u w k the entry's error is at most (C + 3.4) p + 2 q + 4 |p - q|, which is convex
    in (p, q) over [0, 1]^2 and largest in a corner -- C + 7.4 at (1, 0), 6 at (0, 1), C + 5.4 at (1, 1).  So: (C + 9) u w k,
    ce_row_floor's C + 7 with one more rounding for q and one for w; a row of weight 0 has no allowance at all."""
    return (C + 9) * U * np.abs(np.asarray(w, np.float64)) * k


def check_ce(loss, dl, z32, y, label_smoothing, class_weights, grad_scale, what, worst=None):
    """loss: 1e-5 of |ref| (the project's gate for the cross entropy: every term q (lse - z) and every weight is non-negative,
    so the sum does not cancel).  dlogits per row: 1e-5 of the row's own max|ref| + row_floor.  The reference is fp64 of the
    fp32 logits, of float(float32(label_smoothing)) and of the float32 weights -- the numbers the kernel receives.  A label
    outside [0, C): the loss must be NaN.  Returns the reference (loss, dlogits)."""
    eps = float(np.float32(label_smoothing))
    cw = None if class_weights is None else np.asarray(class_weights, np.float32).astype(np.float64)
    z = np.asarray(z32, np.float32).astype(np.float64)
    ref_loss, ref_dl = softmax_ce(z, y, eps, cw, grad_scale)
    _, _, w, P, _, ok = terms(z, y, eps, cw)
    if loss is not None:
        got = float(np.asarray(loss).reshape(-1)[0])
        if not ok.all() and P > 0:
            assert np.isnan(got), "%s: a label outside [0, C) did not poison the loss (%r)" % (what, got)
        else:
            HR.check_close([got], [ref_loss], what + " loss", rel=1e-5, worst=worst)
    if dl is not None:
        dl = np.asarray(dl)
        assert np.isfinite(dl).all(), what + ": dlogits are not finite"
        floor = row_floor(z.shape[1], w, grad_scale / P) if P else np.zeros(z.shape[0])
        HR.check_rows(dl, ref_dl, what + " dlogits per row", 1e-5, floor=floor, worst=worst)
        dead = (w == 0) | (P == 0)
        assert not np.asarray(dl).reshape(ref_dl.shape)[dead].any(), what + ": a row of weight 0 has a non-zero gradient"
    return ref_loss, ref_dl
