"""fp64 restatement of gradient clipping for the tests (tests/test_grad_clip_*.py): what TensorFlow 1.x defines, applied to
the oracle's gradients -- the oracle itself (oracle/) has no clipping.
  tf.clip_by_norm(t, c)          = t * c / max(||t||_2, c)
  tf.clip_by_global_norm(ts, c)  = every t * c / max(sqrt(sum ||t||_2^2), c)
"""
import numpy as np


def flat_indices(seg_row, k0, count):
    """Flat indices of elements k0 .. k0 + count - 1 of a segment (offset, rows, ld, c0, ncols, ...): the kernels' rule."""
    off, rows, ld, c0, ncols = (int(x) for x in seg_row[:5])
    k = np.arange(k0, k0 + count, dtype=np.int64)
    return off + (k // ncols) * ld + c0 + k % ncols


def norms(grads):
    """({name: ||g||_2}, global norm) of a dict of arrays, in fp64."""
    per = {n: float(np.sqrt(np.sum(np.square(np.asarray(g, np.float64))))) for n, g in grads.items()}
    return per, float(np.sqrt(sum(x * x for x in per.values())))


def factors(grads, mode, c):
    """{name: factor}: mode 'variable' (clip_gradient_norm), 'global' (clip_global_norm) or None."""
    per, glob = norms(grads)
    if mode == "variable":
        return {n: c / max(x, c) for n, x in per.items()}
    if mode == "global":
        return {n: c / max(glob, c) for n in per}
    return {n: 1.0 for n in per}


def clipped_adam_step(S, w, g, m, v, t, lr, mode, c):
    """One TF-Adam step (S.adam_step, fp64) of every variable of `g` on the clipped gradients.  w, m, v: dicts of fp64
    arrays, replaced in place.  Returns the factors."""
    f = factors(g, mode, c)
    for n in g:
        w[n], m[n], v[n] = S.adam_step(np.asarray(w[n], np.float64), np.asarray(g[n], np.float64) * f[n], m[n], v[n], t, lr)
    return f
