"""The pooling kernels of csrc/pool.hip against the fp64 oracle (oracle/tf_semantics.py): values, winner bytes, routed
gradient, every dispatch branch, more than one trip through the grid-stride loops, and inputs that TIE.

The winner of a window is its first maximum in row-major order of the padded window, tap index kh*k + kw
(tests/test_oracle_known_answers.py pins that rule on the oracle by hand).  Three separate pieces of code implement it
-- the strict '>' of maxpool_fwd_kernel, the separable kw-then-kh rule of maxpool3_fwd_rolling, the loader of the conv
kernels (tied byte for byte to these in test_kernels_gpu.py) -- and with 16-bit activation storage exact ties among
positive values are routine, so the rule decides where gradients go.

Inputs, two kinds per case:
  ties    np.round(normal(0, 0.3) * 4) / 4: multiples of 0.25, exact in fp32 and bf16; the plain pools (post-ReLU
          consumers) get max(., 0) of it.  Every test asserts on the oracle's own windows that at least a quarter of the
          windows that hold two or more input cells have a duplicated maximum, and for the post-ReLU inputs that at least
          5 % have a duplicated POSITIVE maximum.  (A window with a single cell -- all of case 1x1x1x4 -- cannot tie.)
  normal  continuous normals.
Every input is exactly representable in fp32 (and the bf16 launches of the continuous kind are compared with the oracle
on the bf16-rounded values), so the only error is the kernels' own arithmetic and every tolerance is either exact
equality or an elementwise bound on that arithmetic with u = 2^-24:
  maximum, winner bytes                      exact
  deferred BatchNorm + ReLU pool, fp32       2 u (|max z| rstd + |shift|)      one multiply, one add
  routed gradient                            k^2 u (sum |addends| + |base|)    at most k^2 addends and the base
  mean over HW cells                         HW u (sum |x| / HW)
  gradient of the mean, dropout off          2 ulp of the result               two roundings: 1 / HW, the product
"""
import functools

import numpy as np
import pytest
import torch

from oracle import tf_semantics as S
from test_kernels_gpu import _ops, dev

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
# ds::kMaxStreamBlocks (csrc/ds_common.h: kCUs * 8 = 2048 workgroups) x 256 threads: the work items one pass of a
# grid-stride loop covers.  The product library does not export the constant.
ONE_PASS = 2048 * 256

# (k, stride, mode, (N, H, W, C))
POOL3S1 = [(3, 1, "SAME", s) for s in [(1, 1, 1, 4), (2, 1, 5, 4), (2, 5, 1, 8), (3, 2, 3, 12), (2, 9, 5, 68), (2, 5, 11, 832),
                                       (1, 4, 3, 1024)]]
POOL3S2 = [(3, 2, "SAME", s) for s in [(2, 2, 2, 4), (2, 3, 4, 12), (2, 4, 3, 12), (3, 9, 10, 24), (2, 10, 9, 68), (1, 17, 6, 128),
                                       (2, 5, 8, 8)]]          # both parities of H and of W: pad_t / pad_l 0 and 1, H != W
POOL2S2 = [(2, 2, "SAME", (2, 14, 14, 832)), (2, 2, "SAME", (2, 7, 5, 12)), (2, 2, "VALID", (2, 9, 7, 8))]       # maxpool_fwd_kernel, maxpool_bwd_kernel<2,2>
OTHER = [(2, 1, "SAME", (2, 11, 8, 8)), (5, 3, "SAME", (2, 11, 8, 8))]                                            # maxpool_bwd_kernel<0,0>
POOL3S2_VALID = [(3, 2, "VALID", (2, 9, 9, 12)), (3, 2, "VALID", (2, 11, 8, 12))]                                 # H > 2 OH: maxpool_bwd_kernel<3,2>
CASES = POOL3S1 + POOL3S2 + POOL2S2 + OTHER + POOL3S2_VALID
SAME_CASES = [c for c in CASES if c[2] == "SAME"]

def _id(case):
    k, s, mode, shape = case
    return "%dx%d/%d-%s-%s" % (k, k, s, mode, "x".join(map(str, shape)))


def _out_hw(case):
    k, s, mode, (N, H, W, Cc) = case
    if mode == "SAME":
        return S.same_pad(H, k, s)[0], S.same_pad(W, k, s)[0]
    return (H - k) // s + 1, (W - k) // s + 1


def _f32(a):
    """The values rounded to fp32, as float64 (what the device tensor made from them holds)."""
    return np.asarray(a).astype(np.float32).astype(np.float64)


def _bf16(a):
    return torch.from_numpy(np.asarray(a, dtype=np.float32)).to(torch.bfloat16).to(torch.float64).numpy()


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def tie_counts(x, k, s, mode):
    """(windows holding >= 2 input cells, those with a duplicated maximum, those with a duplicated positive maximum)."""
    win, _, _ = S._patches(x, k, k, s, -np.inf, mode)
    m = win.max(axis=(3, 4))
    can = np.isfinite(win).sum(axis=(3, 4)) >= 2
    dup = ((win == m[:, :, :, None, None, :]).sum(axis=(3, 4)) >= 2) & can
    return int(can.sum()), int(dup.sum()), int((dup & (m > 0)).sum())


def assert_ties_bite(counts, relu):
    can, dup, dup_pos = counts
    assert 4 * dup >= can, "only %d of %d windows tie" % (dup, can)
    if relu:
        assert 20 * dup_pos >= can, "only %d of %d windows tie on a positive maximum" % (dup_pos, can)


def pool_input(case, kind, relu):
    k, s, mode, shape = case
    rng = np.random.RandomState(1000 * (kind == "normal"))        # seed 0: the tie conditions hold for every case (checked on the CPU)
    if kind == "normal":
        return _f32(rng.normal(size=shape))
    x = np.round(rng.normal(scale=0.3, size=shape) * 4) / 4
    return np.maximum(x, 0) if relu else x


@functools.lru_cache(maxsize=None)
def plain_reference(case, kind, dtype):
    """x (what the kernel reads, as float64), the oracle's maxima and winner bytes: computed once, shared, read-only."""
    k, s, mode, shape = case
    x = pool_input(case, kind, relu=True)
    if kind == "ties":
        assert_ties_bite(tie_counts(x, k, s, mode), relu=True)
        assert np.array_equal(_bf16(x), x)                 # multiples of 0.25: nothing is lost in bf16
    elif dtype == "bf16":
        x = _bf16(x)
    return _frozen(x, S.max_pool(x, k, s, mode), S.max_pool_argmax(x, k, s, mode))


def run_fwd(ops, x, case, dtype):
    k, s, mode, (N, H, W, Cc) = case
    OH, OW = _out_hw(case)
    td = torch.bfloat16 if dtype == "bf16" else torch.float32
    xd = dev(x, td)
    assert np.array_equal(xd.double().cpu().numpy(), x)     # the device holds exactly the oracle's input
    y = torch.full((N, OH, OW, Cc), float("nan"), device="cuda", dtype=td)
    am = torch.full((N, OH, OW, Cc), 255, dtype=torch.uint8, device="cuda")
    assert ops.maxpool_fwd(xd, y, am, N, H, W, Cc, k, s, mode) == (OH, OW)
    torch.cuda.synchronize()
    return y, am


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("kind", ["ties", "normal"])
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_max_pool_values_and_winner_bytes_are_the_oracles(case, kind, dtype):
    """ds_maxpool_fwd, fp32 and bf16 storage: y is exactly the window maximum and argmax is S.max_pool_argmax at every
    position (3x3: maxpool3_fwd_rolling<1>, <2>; other windows: maxpool_fwd_kernel)."""
    x, y_ref, arg_ref = plain_reference(case, kind, dtype)
    y, am = run_fwd(_ops(), x, case, dtype)
    assert np.array_equal(y.double().cpu().numpy(), y_ref)
    assert np.array_equal(am.cpu().numpy(), arg_ref)


def bwd_bound(x, dy, base, case, acc):
    """(reference, elementwise bound) of dx = [base +] MaxPoolGrad(x, dy): k^2 u (sum |addends| + |base|)."""
    k, s, mode, _ = case
    ref = S.max_pool_bwd(x, dy, k, s, mode)
    mag = S.max_pool_bwd(x, np.abs(dy), k, s, mode)
    if acc:
        ref, mag = ref + base, mag + np.abs(base)
    return ref, k * k * U * mag


@pytest.mark.parametrize("kind", ["ties", "normal"])
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_max_pool_gradient_against_the_oracle_on_every_dispatch_branch(case, kind):
    """ds_maxpool_bwd on the winners ds_maxpool_fwd wrote, overwriting and accumulating onto a random base:
    maxpool3s1_bwd_rolling (3x3/1 SAME), maxpool3s2_bwd_patch (3x3/2 with H <= 2 OH and W <= 2 OW: the SAME cases, square or
    not, either parity), maxpool_bwd_kernel<3,2> (3x3/2 VALID on 9x9 and 11x8: H > 2 OH), <2,2> and <0,0> (2x2/1, 5x5/3)."""
    ops = _ops()
    k, s, mode, (N, H, W, Cc) = case
    OH, OW = _out_hw(case)
    if k == 3 and s == 2:
        assert (H <= 2 * OH and W <= 2 * OW) == (mode == "SAME")         # which kernel the case reaches
    x, _, arg_ref = plain_reference(case, kind, "f32")
    _, am = run_fwd(ops, x, case, "f32")
    assert np.array_equal(am.cpu().numpy(), arg_ref)
    rng = np.random.RandomState(5)
    dy, base = _f32(rng.normal(size=arg_ref.shape)), _f32(rng.normal(size=x.shape))
    for acc in (False, True):
        dx = dev(base)
        ops.maxpool_bwd(dev(dy), am, dx, acc, N, H, W, Cc, k, s, mode)
        torch.cuda.synchronize()
        ref, bound = bwd_bound(x, dy, base, case, acc)
        err = np.abs(dx.double().cpu().numpy() - ref)
        assert (err <= bound).all(), "accumulate=%s: %.3e over the bound" % (acc, (err - bound).max())


@pytest.mark.parametrize("case", POOL3S1, ids=_id)
def test_max_pool_gradient_variants_equal_the_anchored_one_on_ties(case):
    """ds_maxpool3_bwd_sums (fp32 and bf16 y) is bit-identical to ds_maxpool_bwd -- which the test above anchors -- on
    winners decided by ties."""
    ops = _ops()
    k, s, mode, (N, H, W, Cc) = case
    x, _, arg_ref = plain_reference(case, "ties", "f32")
    pooled, am = run_fwd(ops, x, case, "f32")
    assert np.array_equal(am.cpu().numpy(), arg_ref)
    rng = np.random.RandomState(6)
    dy = dev(rng.normal(size=x.shape))
    base = dev(rng.normal(size=x.shape))
    P = ops.maxpool3_bwd_sums_partials(N, W, Cc)
    assert P >= 1
    for acc in (False, True):
        want = base.clone()
        ops.maxpool_bwd(dy, am, want, acc, N, H, W, Cc, 3, 1, "SAME")
        parts = []
        for y in (pooled, pooled.to(torch.bfloat16)):
            got = base.clone()
            part = torch.full((2, Cc, P), float("nan"), device="cuda")
            ops.maxpool3_bwd_sums(dy, am, got, acc, y, N, H, W, Cc, part)
            torch.cuda.synchronize()
            assert torch.equal(want, got)
            parts.append(part)
        assert torch.equal(parts[0], parts[1])              # the pooled ties are exact in bf16: same y, same sums
        g = (want.double() * (pooled.double() > 0)).reshape(-1, Cc)
        mag = g.abs().sum(0).cpu().numpy()
        # sum g over M = N H W cells in some fixed order, every partial sum below sum |g|: (M - 1) u sum |g|
        err = np.abs(parts[0][0].double().sum(1).cpu().numpy() - g.sum(0).cpu().numpy())
        assert (err <= N * H * W * U * mag).all()


@functools.lru_cache(maxsize=None)
def bn_reference(case, kind):
    k, s, mode, (N, H, W, Cc) = case
    z = pool_input(case, kind, relu=False)
    if kind == "ties":
        assert_ties_bite(tie_counts(z, k, s, mode), relu=False)
    rng = np.random.RandomState(16)
    rstd, shift = _f32(rng.uniform(0.5, 2.0, size=Cc)), _f32(rng.normal(size=Cc) * 0.5)
    return _frozen(z, rstd, shift, S.max_pool(z, k, s, mode), S.max_pool_argmax(z, k, s, mode))


@pytest.mark.parametrize("kind", ["ties", "normal"])
@pytest.mark.parametrize("case", SAME_CASES, ids=_id)
def test_deferred_batch_norm_relu_pool_against_the_oracle(case, kind):
    """ds_maxpool_bn_relu_fwd: the winner is the first maximum of the pre-BatchNorm z (rstd > 0); y = relu(rstd max z +
    shift) within two roundings; the bf16 output is the fp32 one rounded to nearest even; amax is max y; and the gradient
    routed through the winners, masked by relu(bn(z)) > 0, is that of the unfused BatchNorm-ReLU -> MaxPool pair."""
    ops = _ops()
    k, s, mode, (N, H, W, Cc) = case
    OH, OW = _out_hw(case)
    z, rstd, shift, m_ref, arg_ref = bn_reference(case, kind)
    zd, rd, sd = dev(z), dev(rstd), dev(shift)

    def run(td, with_amax):
        y = torch.full((N, OH, OW, Cc), float("nan"), device="cuda", dtype=td)
        am = torch.full((N, OH, OW, Cc), 255, dtype=torch.uint8, device="cuda")
        rec = torch.zeros(ops.AMAX_FLOATS, device="cuda") if with_amax else None
        ops.maxpool_bn_relu_fwd(zd, rd, sd, y, am, N, H, W, Cc, k, s, amax=rec)
        torch.cuda.synchronize()
        return y, am, rec

    y32, am, _ = run(torch.float32, False)
    assert np.array_equal(am.cpu().numpy(), arg_ref)
    y_ref = np.maximum(m_ref * rstd + shift, 0)
    err = np.abs(y32.double().cpu().numpy() - y_ref)
    bound = 2 * U * (np.abs(m_ref) * rstd + np.abs(shift))
    assert (err <= bound).all(), (err - bound).max()
    if k == 3:                                              # the rolling kernels: bf16 output and the max y record
        y32a, am_a, rec = run(torch.float32, True)
        assert torch.equal(y32a, y32) and torch.equal(am_a, am)
        assert ops.amax_value(rec) == float(y32.max())
        for with_amax in (False, True):
            y16, am16, rec = run(torch.bfloat16, with_amax)
            assert torch.equal(y16, y32.to(torch.bfloat16)) and torch.equal(am16, am)
            if with_amax:
                assert ops.amax_value(rec) == float(y32.max())
    y_full = np.maximum(z * rstd + shift, 0)
    rng = np.random.RandomState(7)
    dy = _f32(rng.normal(size=arg_ref.shape))
    dx = torch.full((N, H, W, Cc), float("nan"), device="cuda")
    ops.maxpool_bwd(dev(dy), am, dx, False, N, H, W, Cc, k, s, "SAME")
    torch.cuda.synchronize()
    live = y_full > 0                                       # what BatchNorm backward keeps of it
    want = S.max_pool_bwd(y_full, dy, k, s, "SAME") * live
    bound = k * k * U * S.max_pool_bwd(y_full, np.abs(dy), k, s, "SAME") * live
    err = np.abs(dx.double().cpu().numpy() * live - want)
    assert (err <= bound).all(), (err - bound).max()


# ---- more than one trip through the grid-stride loops ---------------------------------------------------------------
# (case, work items of each kernel it is there for); the rolling kernels keep r0 / r1 / q[] across rows INSIDE that loop
BIG = [
    # maxpool3_fwd_rolling<1> (f32, bf16) and maxpool3s1_bwd_rolling: N * W * C/4 = 125 * 28 * 300 = 1 050 000
    ((3, 1, "SAME", (125, 3, 28, 1200)), lambda N, H, W, OH, OW, C4: (N * OW * C4, N * W * C4)),
    # maxpool3_fwd_rolling<2> (f32, bf16): N * OW * C/4 = 250 * 14 * 300 = 1 050 000;
    # maxpool3s2_bwd_patch: N * (OH + 1) * (OW + 1) * C/4 = 250 * 3 * 15 * 300 = 3 375 000
    ((3, 2, "SAME", (250, 3, 28, 1200)), lambda N, H, W, OH, OW, C4: (N * OW * C4, N * (OH + 1) * (OW + 1) * C4)),
    # maxpool_fwd_kernel (f32, bf16): N * OH * OW * C/4; maxpool_bwd_kernel: N * H * W * C/4; both 42 * 3 * 28 * 300 = 1 058 400
    ((2, 1, "SAME", (42, 3, 28, 1200)), lambda N, H, W, OH, OW, C4: (N * OH * OW * C4, N * H * W * C4)),
]


@functools.lru_cache(maxsize=1)
def big_input(case):
    """Tie-rich post-ReLU input of a large case, fp32; the forward and the gradient part of a case run back to back and share it."""
    x = np.maximum(np.round(np.random.RandomState(3).normal(scale=0.3, size=case[3]) * 4) / 4, 0).astype(np.float32)
    return _frozen(x)[0]


def _slices(N, step=25):
    return [slice(n0, min(N, n0 + step)) for n0 in range(0, N, step)]


@pytest.mark.parametrize("part", ["forward", "gradient"])
@pytest.mark.parametrize("big", BIG, ids=lambda b: _id(b[0]))
def test_pools_over_more_than_one_grid_pass(big, part):
    """Every thread takes at least two trips through its grid-stride loop (at most ds::kMaxStreamBlocks workgroups of 256):
    forward in fp32 and bf16 storage, gradient overwriting and accumulating, on tie-rich input, with the assertions of
    the small cases.  Images are independent: the oracle runs on a few at a time."""
    ops = _ops()
    case, items = big
    k, s, mode, (N, H, W, Cc) = case
    OH, OW = _out_hw(case)
    assert min(items(N, H, W, OH, OW, Cc // 4)) >= 2 * ONE_PASS
    x = big_input(case)
    xd = torch.from_numpy(x).cuda()
    y = torch.full((N, OH, OW, Cc), float("nan"), device="cuda")
    am = torch.full((N, OH, OW, Cc), 255, dtype=torch.uint8, device="cuda")
    ops.maxpool_fwd(xd, y, am, N, H, W, Cc, k, s, mode)
    if part == "forward":
        y16, am16 = y.to(torch.bfloat16).fill_(float("nan")), am.clone().fill_(255)
        ops.maxpool_fwd(xd.to(torch.bfloat16), y16, am16, N, H, W, Cc, k, s, mode)
        torch.cuda.synchronize()
        assert torch.equal(y16.float(), y) and torch.equal(am16, am)       # multiples of 0.25: bf16 storage loses nothing
        y, am = y.cpu().numpy(), am.cpu().numpy()
        counts = np.zeros(3, dtype=np.int64)
        for sl in _slices(N):
            xs = x[sl].astype(np.float64)
            counts += tie_counts(xs, k, s, mode)
            assert np.array_equal(y[sl], S.max_pool(xs, k, s, mode)), sl
            assert np.array_equal(am[sl], S.max_pool_argmax(xs, k, s, mode)), sl
        assert_ties_bite(counts, relu=True)
        return
    # the gradient through the winners of the launch above (the forward part holds them to the oracle's)
    rng = np.random.RandomState(4)
    dy = (rng.randint(-2 ** 20, 2 ** 20, size=(N, OH, OW, Cc)) / 2.0 ** 18).astype(np.float32)        # uniform in [-4, 4), exact in fp32
    base = (rng.randint(-2 ** 20, 2 ** 20, size=(N, H, W, Cc)) / 2.0 ** 18).astype(np.float32)
    dyd, dxs = torch.from_numpy(dy).cuda(), []
    for acc in (False, True):
        dx = torch.from_numpy(base).cuda()
        ops.maxpool_bwd(dyd, am, dx, acc, N, H, W, Cc, k, s, mode)
        dxs.append(dx)
    torch.cuda.synchronize()
    dxs = [d.cpu().numpy() for d in dxs]
    for sl in _slices(N):
        xs, dys, bs = x[sl].astype(np.float64), dy[sl].astype(np.float64), base[sl].astype(np.float64)
        ref = S.max_pool_bwd(xs, dys, k, s, mode)
        mag = S.max_pool_bwd(xs, np.abs(dys), k, s, mode)
        assert (np.abs(dxs[0][sl] - ref) <= k * k * U * mag).all(), sl
        assert (np.abs(dxs[1][sl] - (ref + bs)) <= k * k * U * (mag + np.abs(bs))).all(), sl


# ---- 7x7 average pool + dropout ---------------------------------------------------------------------------------------
AVG_SHAPES = [(3, 49, 1028), (1, 1, 4), (2, 7, 2052)]      # (N, HW, C): two and three trips of the c += 1024 loop, the last ragged; HW = 1


def _avg_inputs(shape):
    N, HW, Cc = shape
    rng = np.random.RandomState(9)
    return _f32(rng.normal(size=(N, HW, Cc))), _f32(rng.normal(size=(N, Cc))), (rng.uniform(size=(N, Cc)) < 0.8).astype(np.float64)


@pytest.mark.parametrize("shape", AVG_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_avgpool_with_dropout_off(shape):
    """keep = 1: out is the plain mean (HW additions and the scaling: HW u sum |x| / HW), mask_out is all ones, the seed does
    not matter; the backward never reads its mask (a NaN-filled one is passed) and is d / HW within two roundings."""
    ops = _ops()
    N, HW, Cc = shape
    x, d, _ = _avg_inputs(shape)
    xd = dev(x)
    outs = []
    for seed in (0, 12345):
        out, mo = torch.full((N, Cc), float("nan"), device="cuda"), torch.full((N, Cc), float("nan"), device="cuda")
        ops.avgpool_dropout_fwd(xd, N, HW, Cc, 1.0, seed, None, mo, out)
        torch.cuda.synchronize()
        assert torch.equal(mo, torch.ones_like(mo))
        outs.append(out)
    assert torch.equal(outs[0], outs[1])
    err = np.abs(outs[0].double().cpu().numpy() - x.mean(1))
    assert (err <= HW * U * np.abs(x).sum(1) / HW).all()
    dx = torch.full((N, HW, Cc), float("nan"), device="cuda")
    ops.avgpool_dropout_bwd(dev(d), torch.full((N, Cc), float("nan"), device="cuda"), N, HW, Cc, 1.0, dx)
    torch.cuda.synchronize()
    ref = np.broadcast_to((d / HW)[:, None, :], (N, HW, Cc))
    got = dx.double().cpu().numpy()
    assert np.isfinite(got).all()
    assert (np.abs(got - ref) <= 2 * np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)).all()


@pytest.mark.parametrize("shape", AVG_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_avgpool_dropout_with_a_given_mask_over_several_channel_trips(shape):
    """keep = 0.8 and an injected mask on the shapes above.  Forward: the mean as before, then m / keep and one more product
    -- (HW + 3) u sum |x| / HW scale.  Backward: d * m is exact, scale = (1 / keep) / HW is two roundings, the product a third: 3 u."""
    ops = _ops()
    N, HW, Cc = shape
    x, d, mask = _avg_inputs(shape)
    keep = float(np.float32(0.8))
    out, mo = torch.full((N, Cc), float("nan"), device="cuda"), torch.full((N, Cc), float("nan"), device="cuda")
    ops.avgpool_dropout_fwd(dev(x), N, HW, Cc, 0.8, 0, dev(mask), mo, out)
    torch.cuda.synchronize()
    assert np.array_equal(mo.double().cpu().numpy(), mask)
    err = np.abs(out.double().cpu().numpy() - x.mean(1) * mask / keep)
    assert (err <= (HW + 3) * U * np.abs(x).sum(1) / HW * mask / keep).all()
    dx = torch.full((N, HW, Cc), float("nan"), device="cuda")
    ops.avgpool_dropout_bwd(dev(d), dev(mask), N, HW, Cc, 0.8, dx)
    torch.cuda.synchronize()
    ref = np.broadcast_to((d * mask / keep / HW)[:, None, :], (N, HW, Cc))
    assert (np.abs(dx.double().cpu().numpy() - ref) <= 3 * U * np.abs(ref)).all()


@pytest.mark.parametrize("shape", AVG_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_avgpool_dropout_device_seed_counter_adds_to_the_host_seed(shape):
    """seed_dev: a device counter d added to the host seed draws the mask of host seed + d."""
    ops = _ops()
    N, HW, Cc = shape
    x, _, _ = _avg_inputs(shape)
    xd = dev(x)
    seed, d = 1000, 77

    def run(seed, counter):
        out, mo = torch.full((N, Cc), float("nan"), device="cuda"), torch.full((N, Cc), float("nan"), device="cuda")
        ops.avgpool_dropout_fwd(xd, N, HW, Cc, 0.8, seed, None, mo, out, seed_dev=counter)
        torch.cuda.synchronize()
        return out, mo

    out_dev, m_dev = run(seed, torch.tensor([d], dtype=torch.int64, device="cuda"))
    out_host, m_host = run(seed + d, None)
    assert torch.equal(m_dev, m_host) and torch.equal(out_dev, out_host)
    assert bool(((m_dev == 0) | (m_dev == 1)).all())
    _, m_zero = run(seed, torch.zeros(1, dtype=torch.int64, device="cuda"))
    _, m_plain = run(seed, None)
    assert torch.equal(m_zero, m_plain)
    if N * Cc >= 1000:
        assert not torch.equal(m_dev, m_plain)              # the counter is read
        assert abs(float(m_dev.mean()) - 0.8) < 0.05


def test_avgpool_dropout_gradient_over_more_than_one_grid_pass():
    """avgpool_dropout_bwd_kernel: N * HW * C/4 = 84 * 49 * 257 = 1 057 812 work items, with the mask and without."""
    ops = _ops()
    N, HW, Cc = 84, 49, 1028
    assert N * HW * (Cc // 4) >= 2 * ONE_PASS
    rng = np.random.RandomState(11)
    d = _f32(rng.normal(size=(N, Cc)))
    mask = (rng.uniform(size=(N, Cc)) < 0.8).astype(np.float64)
    keep = float(np.float32(0.8))
    for kp, md, ref, tol in ((0.8, dev(mask), d * mask / keep / HW, 3 * U),
                             (1.0, torch.full((N, Cc), float("nan"), device="cuda"), d / HW, 2 * U)):
        dx = torch.full((N, HW, Cc), float("nan"), device="cuda")
        ops.avgpool_dropout_bwd(dev(d), md, N, HW, Cc, kp, dx)
        torch.cuda.synchronize()
        got = dx.double().cpu().numpy()
        assert (np.abs(got - ref[:, None, :]) <= tol * np.abs(ref)[:, None, :]).all()
