"""The optimisers of slim's --optimizer and its learning-rate schedules restated for the tests, independent of the package's
own helpers.  [TF-sem]: TensorFlow is not in the reference tree; these are TF 1.x's training_ops CPU functors
(ApplyGradientDescent, ApplyMomentum with use_nesterov=False, ApplyRMSProp, ApplyAdam) and tf.train.exponential_decay /
polynomial_decay restated, parity unpinned.

    g_eff     gi = g * grad_scale; on the first n_wd elements gi = gi + wd * w; clipped: gi = gi * factor
    sgd       p = lr*gi; theta = w - p
    momentum  t = mu*acc; a = t + gi; acc = a; p = lr*a; theta = w - p
    rmsprop   q = gi*gi; d = q - ms; e = d*(1 - rho); ms' = ms + e; s = sqrt(ms' + eps); nmr = gi*lr; r = nmr / s;
              t = mom*mu; mom' = t + r; theta = w - mom'
    adam      m' = b1*m + (1 - b1)*gi; v' = b2*v + ((1 - b2)*gi)*gi; theta = w - (lr_t*m') / (sqrt(v') + eps)

in fp32 operation by operation (NumPy never contracts; what the kernels must give bit for bit where +, -, * are the only
operations) and in fp64 on the same fp32 inputs (what they are bounded against)."""
from fractions import Fraction

import numpy as np

U = 2.0 ** -24      # unit roundoff of fp32
f32 = np.float32


def _a32(*xs):
    return [np.asarray(x, np.float32) for x in xs]


def g_eff32(theta, g, n_wd, wd, scale, factor=None):
    """The effective gradient as the kernels form it: a product, on the L2 part a product and a sum, clipped one more product."""
    theta, g = _a32(theta, g)
    gi = (g * f32(scale)).astype(np.float32)
    gi[:n_wd] = gi[:n_wd] + (f32(wd) * theta[:n_wd]).astype(np.float32)
    if factor is not None:
        gi = (gi * np.asarray(factor, np.float32)).astype(np.float32)
    return gi


def sgd32(theta, gi, lr):
    theta, gi = _a32(theta, gi)
    p = (f32(lr) * gi).astype(np.float32)
    return (theta - p).astype(np.float32)


def momentum32(theta, acc, gi, lr, mu):
    """(theta', acc')"""
    theta, acc, gi = _a32(theta, acc, gi)
    t = (f32(mu) * acc).astype(np.float32)
    a = (t + gi).astype(np.float32)
    p = (f32(lr) * a).astype(np.float32)
    return (theta - p).astype(np.float32), a


def rmsprop32(theta, mom, ms, gi, lr, mu, rho, eps):
    """(theta', mom', ms')"""
    theta, mom, ms, gi = _a32(theta, mom, ms, gi)
    q = (gi * gi).astype(np.float32)
    d = (q - ms).astype(np.float32)
    e = (d * f32(f32(1.0) - f32(rho))).astype(np.float32)
    msn = (ms + e).astype(np.float32)
    s = np.sqrt((msn + f32(eps)).astype(np.float32)).astype(np.float32)
    nmr = (gi * f32(lr)).astype(np.float32)
    r = (nmr / s).astype(np.float32)
    t = (mom * f32(mu)).astype(np.float32)
    momn = (t + r).astype(np.float32)
    return (theta - momn).astype(np.float32), momn, msn


def adam32(theta, m, v, gi, lr_t, b1, b2, eps):
    """(theta', m', v')"""
    theta, m, v, gi = _a32(theta, m, v, gi)
    mi = ((f32(b1) * m).astype(np.float32) + (f32(f32(1.0) - f32(b1)) * gi).astype(np.float32)).astype(np.float32)
    vi = ((f32(b2) * v).astype(np.float32) +
          ((f32(f32(1.0) - f32(b2)) * gi).astype(np.float32) * gi).astype(np.float32)).astype(np.float32)
    den = (np.sqrt(vi).astype(np.float32) + f32(eps)).astype(np.float32)
    wn = (theta - ((f32(lr_t) * mi).astype(np.float32) / den).astype(np.float32)).astype(np.float32)
    return wn, mi, vi


# ---- fp64 on the fp32 inputs, with a running forward error bound of the fp32 chain -----------------------------------------
# A quantity is a pair (x, E): x the value of the chain in exact arithmetic -- evaluated in fp64, whose own rounding (2^-53
# per operation) is covered by the 1.001 below -- and E a bound on |x_fp32 - x|.  Inputs are exact (E = 0).  Every fp32
# operation returns fl(y) with |fl(y) - y| <= u |y| (no underflow: the test magnitudes keep every intermediate above 1e-30),
# so with P = the error its operands carry into y and |y_fp32 operands' result| <= |y| + P:
#     add / sub   P = Ea + Eb                                   E = P + u (|y| + P)
#     mul         P = |a| Eb + |b| Ea + Ea Eb                   E = P + u (|y| + P)
#     div         P = (Ea + |y| Eb) / (|b| - Eb)   (Eb < |b|)   E = P + u (|y| + P)
#     sqrt        P = Ea / (2 sqrt(a - Ea))        (Ea < a: the slope of sqrt between a - Ea and a + Ea is at most that;
#                                                   Ea = 0, an exact operand such as a zero pad element: P = 0)
#                                                               E = P + u (|y| + P)
# one u |result| per rounded operation, propagated through what follows.  The bound of an output is 1.001 E.
class Q:
    def __init__(self, x, e=0.0):
        self.x = np.asarray(x, np.float64)
        self.e = np.zeros_like(self.x) + e

    @staticmethod
    def _of(v):
        return v if isinstance(v, Q) else Q(np.float64(f32(v)))

    def _round(self, y, p):
        return Q(y, p + U * (np.abs(y) + p))

    def __add__(self, o):
        o = Q._of(o)
        return self._round(self.x + o.x, self.e + o.e)

    def __sub__(self, o):
        o = Q._of(o)
        return self._round(self.x - o.x, self.e + o.e)

    def __mul__(self, o):
        o = Q._of(o)
        return self._round(self.x * o.x, np.abs(self.x) * o.e + np.abs(o.x) * self.e + self.e * o.e)

    def __truediv__(self, o):
        o = Q._of(o)
        assert (o.e < np.abs(o.x)).all()
        y = self.x / o.x
        return self._round(y, (self.e + np.abs(y) * o.e) / (np.abs(o.x) - o.e))

    def sqrt(self):
        exact = self.e == 0      # (an exact operand, a zero pad element among them: only the root's own rounding)
        assert ((self.e < self.x) | (exact & (self.x >= 0))).all()
        return self._round(np.sqrt(self.x), np.where(exact, 0.0, self.e / (2.0 * np.sqrt(np.where(exact, 1.0, self.x - self.e)))))

    @property
    def bound(self):
        return 1.001 * self.e


def sgd64(theta, gi, lr):
    """theta' as a Q (value in fp64, .bound the forward error bound of sgd32)."""
    return Q(theta) - Q._of(lr) * Q(gi)


def momentum64(theta, acc, gi, lr, mu):
    a = Q._of(mu) * Q(acc) + Q(gi)
    return Q(theta) - Q._of(lr) * a, a


def rmsprop64(theta, mom, ms, gi, lr, mu, rho, eps):
    gi, ms = Q(gi), Q(ms)
    msn = ms + (gi * gi - ms) * (Q._of(1.0) - Q._of(rho))
    r = (gi * Q._of(lr)) / (msn + Q._of(eps)).sqrt()
    momn = Q(mom) * Q._of(mu) + r
    return Q(theta) - momn, momn, msn


def adam64(theta, m, v, gi, lr_t, b1, b2, eps):
    gi = Q(gi)
    mi = Q._of(b1) * Q(m) + (Q._of(1.0) - Q._of(b1)) * gi
    vi = Q._of(b2) * Q(v) + ((Q._of(1.0) - Q._of(b2)) * gi) * gi
    return Q(theta) - (Q._of(lr_t) * mi) / (vi.sqrt() + Q._of(eps)), mi, vi


def worst_ratio(got32, q):
    """max |got - exact| / bound (a zero bound with a zero error counts as 0)."""
    err = np.abs(np.asarray(got32, np.float64) - q.x)
    b = q.bound
    return float(np.max(np.where(err == 0, 0.0, err / np.where(b > 0, b, np.finfo(np.float64).tiny))))


# ---- learning-rate schedules ------------------------------------------------------------------------------------------------
SCHEDULE_DEFAULTS = {"learning_rate_decay_factor": 0.94, "num_epochs_per_decay": 2.0, "end_learning_rate": 1e-4}


def decay_steps(config, num_samples):
    """slim's formula taken literally: int(num_samples / batch_size * num_epochs_per_decay)."""
    return int(num_samples / config["batch_size"] * config.get("num_epochs_per_decay", 2.0))


def schedule32(config, num_samples, t):
    """tf.train.exponential_decay(staircase=True) / polynomial_decay(power=1, cycle=False) / a constant, the way TF forms
    them: every scalar cast to fp32, every operation rounded to fp32 once (the power correctly rounded)."""
    kind = config["learning_rate_decay_type"]
    lr0 = f32(config["initial_lr"])
    if kind == "fixed":
        return lr0
    gs, ds = f32(t), f32(decay_steps(config, num_samples))
    if kind == "exponential":
        p = np.floor(f32(gs / ds))
        factor = f32(config.get("learning_rate_decay_factor", 0.94))
        return f32(lr0 * f32(np.float64(factor) ** np.float64(p)))
    assert kind == "polynomial"
    end = f32(config.get("end_learning_rate", 1e-4))
    p = f32(min(gs, ds) / ds)
    return f32(f32(f32(lr0 - end) * f32(f32(1.0) - p)) + end)


def schedule_exact(config, num_samples, t):
    """The closed form in exact rational arithmetic on the fp32 hyper-parameters (TF holds them as fp32 tensors)."""
    kind = config["learning_rate_decay_type"]
    lr0 = Fraction(float(f32(config["initial_lr"])))
    if kind == "fixed":
        return lr0
    ds = decay_steps(config, num_samples)
    if kind == "exponential":
        return lr0 * Fraction(float(f32(config.get("learning_rate_decay_factor", 0.94)))) ** (t // ds)
    end = Fraction(float(f32(config.get("end_learning_rate", 1e-4))))
    return (lr0 - end) * (1 - Fraction(min(t, ds), ds)) + end


def ulps32(x, exact):
    """|x - exact| in units of the fp32 spacing at `exact`."""
    x = Fraction(float(x))
    return float(abs(x - exact) / Fraction(float(np.spacing(f32(float(exact))))))
