"""tf.train.ExponentialMovingAverage restated for the tests (TensorFlow is not in the reference tree; TF 1.x,
moving_averages.assign_moving_average with zero_debias off), independent of the package's own helpers:

    decay_t = min(decay, (1 + t) / (10 + t))        t = num_updates = 1, 2, ...
    shadow  = shadow - (shadow - variable) * (1 - decay_t)

in fp32 operation by operation (what the kernels must give bit for bit) and in fp64 (what they are bounded against)."""
from fractions import Fraction

import numpy as np

U = 2.0 ** -24      # unit roundoff of fp32


def decay_exact(decay, t):
    """min(decay, (1 + t) / (10 + t)) as an exact rational of the double `decay`."""
    return min(Fraction(float(decay)), Fraction(1 + t, 10 + t))


def decay32(decay, t):
    """decay_t rounded once to fp32: the min in double on the host, then the cast."""
    return np.float32(min(float(decay), (1.0 + t) / (10.0 + t)))


def rate32(decay, t):
    """1 - decay_t formed in fp32, as TF forms it from its fp32 decay tensor."""
    return np.float32(np.float32(1.0) - decay32(decay, t))


def update32(shadow, theta_new, rate):
    """shadow - (shadow - theta_new) * rate: three fp32 operations, each rounded once (NumPy never contracts)."""
    shadow, theta_new = np.asarray(shadow, np.float32), np.asarray(theta_new, np.float32)
    rate = np.float32(rate)
    d = (shadow - theta_new).astype(np.float32)
    p = (d * rate).astype(np.float32)
    return (shadow - p).astype(np.float32)


def update64(shadow, theta_new, rate):
    """The same update in fp64 on the fp32 inputs and the fp32 rate: the exact result to 2^-53."""
    s, w = np.asarray(shadow, np.float64), np.asarray(theta_new, np.float64)
    return s - (s - w) * float(np.float32(rate))


def bound64(shadow, theta_new, rate):
    """|fp32 result - exact| <= 1.001 u (|exact| + 2 rate |s - w|): one rounding of the result, and the roundings of the
    difference and of the product, both of which reach the result through the product."""
    s, w = np.asarray(shadow, np.float64), np.asarray(theta_new, np.float64)
    r = float(np.float32(rate))
    return 1.001 * U * (np.abs(update64(shadow, theta_new, rate)) + 2.0 * r * np.abs(s - w))


class Recurrence:
    """The shadows of a run, advanced in fp32 from the net's own theta after every step."""

    def __init__(self, decay, theta0):
        self.decay, self.t = decay, 0
        self.shadow = np.asarray(theta0, np.float32).copy()

    def step(self, theta_new, skipped=False):
        self.t += 1      # (a skipped step still counts)
        if not skipped:
            self.shadow = update32(self.shadow, theta_new, rate32(self.decay, self.t))
        return self.shadow
