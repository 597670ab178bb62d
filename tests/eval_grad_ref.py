"""Test helper: NumPy fp64 references of the moving-statistics backward kernels (ds_bn_infer_bwd_apply,
ds_bn_pool_infer_bwd_apply, ds_token_dot), shared by tests/test_eval_gradients_cpu.py (which checks the formula against
torch.autograd) and tests/test_eval_gradients_gpu.py (which checks the kernels against the formula)."""
import numpy as np


def bn_infer_relu_bwd(z, dy, rstd, shift):
    """dz of y = relu(z * rstd + shift) (BatchNorm with fixed statistics folded into rstd / shift), per channel on the last
    axis: dz = rstd * dy * [z * rstd + shift > 0], in float64."""
    z, dy, rstd, shift = (np.asarray(a, dtype=np.float64) for a in (z, dy, rstd, shift))
    return rstd * dy * (z * rstd + shift > 0)


def maxpool3s2_bwd(dpool, argmax, H, W):
    """MaxPoolGrad of a 3x3 / 2 SAME pool from the arg-max record (tap = 3 * dy + dx of the winner in its window), NHWC."""
    N, OH, OW, C = dpool.shape
    pad_t = max((OH - 1) * 2 + 3 - H, 0) // 2
    pad_l = max((OW - 1) * 2 + 3 - W, 0) // 2
    g = np.zeros((N, H, W, C), np.float64)
    for oh in range(OH):
        for ow in range(OW):
            for tap in range(9):
                ih, iw = 2 * oh - pad_t + tap // 3, 2 * ow - pad_l + tap % 3
                if 0 <= ih < H and 0 <= iw < W:
                    g[:, ih, iw, :] += np.where(argmax[:, oh, ow, :] == tap, dpool[:, oh, ow, :], 0.0)
    return g


def token_dot(dx, x, seq_len, B, T):
    """out[b, t] = sum_d dx[t*B + b, d] * x[t*B + b, d], 0 at t >= seq_len[b]; time-major [T*B, D] inputs, float64."""
    D = dx.shape[1]
    p = (np.asarray(dx, np.float64) * np.asarray(x, np.float64)).sum(1).reshape(T, B).T
    return np.where(np.arange(T)[None, :] < np.asarray(seq_len)[:, None], p, 0.0)
