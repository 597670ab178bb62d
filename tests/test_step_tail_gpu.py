"""The step tail's kernels (csrc/text_misc.hip: ds_adam_tf, ds_sumsq, ds_colsum, ds_softmax_ce, ds_slab_epilogue_ce, the
step-wise LSTM cell, ds_copy2d / ds_fill / ds_pad_channels) against fp64 evaluations of the same fp32 inputs, at the sizes where
their launch forms change: one element, one short of / one past a workgroup, the grid-stride caps (ds::stream_grid: 2048
workgroups x 256 threads = 524 288 elements; ds_sumsq: 256 workgroups), ds_colsum's one-launch / two-stage switch at 512 rows,
the second trip of the one-workgroup cross entropy past 256 rows.

The tolerances are rounding counts (u = 2^-24, first order), derived in each test's docstring; none was measured.  Each test
prints its worst error / bound ratio.  On an MI355X: ds_adam_tf 0.49 (n = 1) to 0.996 (theta's own final rounding, up to
u |theta|, is nearly all of its bound), ds_sumsq <= 0.088, ds_colsum <= 0.093, ds_softmax_ce <= 0.124,
ds_slab_epilogue_ce <= 0.30 (the logits), the LSTM cell <= 0.013 of its 1e-5 gate; the file takes 6.3 s."""
import numpy as np
import pytest
import torch

import head_ref as HR
from oracle import tf_semantics as S

pytestmark = pytest.mark.gpu

U = HR.U
NAN = float("nan")
CAP = 2048 * 256            # elements one trip of a ds::stream_grid(n, 256) launch covers
GUARD = 7.0


def _ops():
    from tumblr_emotions_amd import ops
    return ops


def dev(a, dtype=torch.float32):
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda")


def host(t):
    return t.detach().cpu().numpy().copy()


def _guarded(a, extra=32):
    """device copy of the flat fp32 array `a` with `extra` guard elements behind it"""
    return dev(np.concatenate([np.asarray(a, np.float32).reshape(-1), np.full(extra, GUARD, np.float32)]))


# ---- ds_adam_tf ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 3, 1003, CAP, CAP + 5, 3 * CAP + 7])
def test_adam_tf_every_boundary_and_both_step_size_forms(n):
    """Three TF-Adam steps with grad_scale 0.5, n_wd in {0, 1, n - 1, n}, the step size from the host and from the device word
    (the host value is then a poison).  Every step is checked from the kernel's own previous fp32 state against one fp64 step
    (head_ref.adam_ref, which derives the per-element bounds: one rounding of theta plus 11.5 u -- plus the denominator's
    cancellation term -- times the magnitude bound of the update, 4 u of m's terms, 8 u of v's).  Around n_wd the gradients are
    zero: undecayed entries must keep the bits of theta and m = v = 0, decayed ones move by about lr, so a boundary off by one
    is an lr-sized error (tests/test_head_ref_cpu.py plants it).  (With a gradient of wd w at every step m_t = wd w (1 - b1^t),
    v_t = (wd w)^2 (1 - b2^t), and the step is lr / (1 + eps / (sqrt(1 - b2^t) wd |w|)) >= 0.98 lr at |w| >= 0.5; the test
    asks for lr / 4.)  The 32 elements behind n stay untouched."""
    ops = _ops()
    worst = HR.Worst()
    hyper = dict(wd=S.WEIGHT_DECAY, grad_scale=0.5, b1=S.ADAM_B1, b2=S.ADAM_B2, eps=S.ADAM_EPS)
    for n_wd in sorted({0, min(1, n), n - 1, n}):
        for on_device in (False, True):
            w, gs = HR.adam_inputs(n, n_wd, seed=n % 1000 + n_wd % 1000)
            theta, m, v = _guarded(w), _guarded(np.zeros(n)), _guarded(np.zeros(n))
            state = (w, np.zeros(n, np.float32), np.zeros(n, np.float32))
            for t in (1, 2, 3):
                lr_t = float(np.float32(1e-3 * np.sqrt(1 - S.ADAM_B2 ** t) / (1 - S.ADAM_B1 ** t)))
                lr_dev = dev([lr_t]) if on_device else None
                ops.adam_tf(theta, dev(gs[t - 1]), m, v, n, n_wd, hyper["wd"], hyper["grad_scale"], 1e3 if on_device else lr_t,
                            hyper["b1"], hyper["b2"], hyper["eps"], lr_t_dev=lr_dev)
                torch.cuda.synchronize()
                full = [host(a) for a in (theta, m, v)]
                what = "adam n=%d n_wd=%d lr_t %s step %d" % (n, n_wd, "on device" if on_device else "from host", t)
                assert all((a[n:] == GUARD).all() for a in full), what + ": wrote past n"
                got = tuple(a[:n] for a in full)
                HR.check_adam(got, state, gs[t - 1], n_wd, lr_t=lr_t, what=what, worst=worst, **hyper)
                if n_wd > 0:      # the decayed zero-gradient entries really move (by about lr_t * m / sqrt(v) = lr)
                    lo = max(0, n_wd - 16)
                    moved = np.abs(got[0][lo:n_wd].astype(np.float64) - state[0][lo:n_wd])
                    assert moved.min() > 0.25e-3, what
                state = got
    print("ds_adam_tf n=%d: %s" % (n, worst))


# ---- ds_sumsq -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 255, CAP, CAP + 1, 3 * CAP + 7])
def test_sumsq_across_its_block_cap(n):
    """min(ceil(n / 2048), 256) workgroups of 256 threads: a thread adds ceil(n / threads) squares serially (one rounding
    each, the first exact), the workgroup's tree has depth 8, the second stage adds the partials in double; with the rounding
    of the squares and of the final cast: |err| <= (serial + 8 + 2) u sum(x^2).  Magnitudes over six decades; two runs give the
    same bits; the scratch holds NaN before."""
    ops = _ops()
    rng = np.random.RandomState(n % 977)
    x = (rng.normal(size=n) * 10.0 ** rng.uniform(-3, 3, size=n)).astype(np.float32)
    blocks = min(-(-n // 2048), 256)
    serial = -(-n // (blocks * 256))
    ref = float((x.astype(np.float64) ** 2).sum())
    xd, outs = _guarded(x), []
    for _ in range(2):
        scratch, out = torch.full((256,), NAN, device="cuda"), torch.full((2,), GUARD, device="cuda")
        ops.sumsq(xd, n, scratch, out)
        torch.cuda.synchronize()
        outs.append(host(out))
    HR.check_bits(outs[0], outs[1], "ds_sumsq twice")
    assert outs[0][1] == GUARD
    worst = HR.Worst()
    HR.check_bound(outs[0][:1], [ref], (serial + 10) * U * ref, "ds_sumsq n=%d" % n, worst)
    print("ds_sumsq n=%d (%d workgroups, %d terms per thread): %s" % (n, blocks, serial, worst))


# ---- ds_colsum ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("M", [1, 3, 512, 513, 4097])
def test_colsum_both_forms_strided_and_cancelling(M):
    """RS = min(ceil(M / 64), 64) row splits of rps = ceil(M / RS) rows; a lane adds every fourth row of its split serially
    (ceil(rps / 4) terms), the four lanes are added (3 roundings), the splits in double, the result is cast (1):
    |err| <= (ceil(rps / 4) + 4) u sum|x| per column.  RS <= 8 (M <= 512) is the one-launch form.  The columns are centred, so
    their sums are rounding-sized against sum|x|; with ld = C + 3 the three columns past C hold 1e30, which no sum may see.  Two
    runs give the same bits; scratch and output hold NaN before."""
    ops = _ops()
    RS = min(-(-M // 64), 64)
    serial = -(-(-(-M // RS)) // 4)
    worst = HR.Worst()
    for C_ in (1, 15, 64, 65, 130):
        for ld in (C_, C_ + 3):
            rng = np.random.RandomState(M + 7 * C_ + ld)
            r = rng.normal(size=(M, C_)) * 10.0 ** rng.uniform(-1, 1, size=(1, C_))
            x = np.full((M, ld), 1e30, np.float32)
            x[:, :C_] = r - (r.mean(0, keepdims=True) if M > 1 else 0.0)
            xd, outs = dev(x), []
            for _ in range(2):
                scratch, out = torch.full((64 * C_,), NAN, device="cuda"), torch.full((C_ + 4,), NAN, device="cuda")
                out[C_:] = GUARD
                ops.colsum(xd, M, C_, ld, scratch, out)
                torch.cuda.synchronize()
                outs.append(host(out))
            what = "ds_colsum M=%d C=%d ld=%d" % (M, C_, ld)
            HR.check_bits(outs[0], outs[1], what + " twice")
            assert (outs[0][C_:] == GUARD).all(), what + ": wrote past C"
            x64 = x[:, :C_].astype(np.float64)
            HR.check_bound(outs[0][:C_], x64.sum(0), (serial + 4) * U * np.abs(x64).sum(0), what, worst)
    print("ds_colsum M=%d (%s, %d rows per lane): %s" % (M, HR.colsum_form(M), serial, worst))


# ---- ds_softmax_ce ------------------------------------------------------------------------------------------------------------

def _ce_ref(z32, y, k):
    """fp64 cross entropy of fp32 logits: (mean loss, softmax, dlogits = (softmax - onehot) k); labels outside [0, C) have an
    all-zero one-hot row (and make the kernel's loss NaN)."""
    z = z32.astype(np.float64)
    B = z.shape[0]
    m = z.max(1, keepdims=True)
    e = np.exp(z - m)
    s = e.sum(1, keepdims=True)
    p = e / s
    ok = (y >= 0) & (y < z.shape[1])
    onehot = np.zeros_like(z)
    onehot[np.arange(B)[ok], y[ok]] = 1.0
    loss = float(np.mean((m[:, 0] + np.log(s[:, 0]) - z[np.arange(B), np.where(ok, y, 0)])[ok])) if ok.all() else NAN
    return loss, p, (p - onehot) * k


def _ce_check(loss, dl, z32, y, k, what, worst):
    """loss: the existing test's gate, 1e-5 of |ref|.  dlogits per row: 1e-5 of the row's own max|ref| (the gate of
    test_softmax_ce_and_adam_and_reductions, per row) + HR.ce_row_floor(C, k), the absolute rounding of (softmax - onehot) k:
    where the label takes nearly all the probability the whole row is smaller than the rounding of softmax itself."""
    ref_loss, _, ref_dl = _ce_ref(z32, y, k)
    if loss is not None:
        HR.check_close(loss, [ref_loss], what + " loss", rel=1e-5, worst=worst)
    if dl is not None:
        HR.check_rows(dl, ref_dl, what + " dlogits per row", 1e-5, floor=HR.ce_row_floor(z32.shape[1], k), worst=worst)


@pytest.mark.parametrize("B", [1, 255, 256, 257, 513])
def test_softmax_ce_rows_classes_and_poisoned_labels(B):
    """One workgroup, thread t takes rows t, t + 256, ...: B crosses one and two trips.  Logits uniform over +-60 (most
    exponentials underflow), one row of equal logits, the upstream scale on the device (1.5 from the host x 0.5), either output
    NULL (the other keeps its bits), and one label outside [0, C): the loss is NaN, that row's dlogits are finite and equal
    softmax x k as the kernel's comment states, every other row keeps its bits."""
    ops = _ops()
    worst = HR.Worst()
    up = dev([0.5])
    for C_ in (1, 2, 15, 32, 33):
        rng = np.random.RandomState(B + 13 * C_)
        for equal_row in ([None, 0] if B == 1 else [B // 2]):
            z = rng.uniform(-60, 60, size=(B, C_)).astype(np.float32)
            if equal_row is not None:
                z[equal_row] = z[equal_row, 0]
            y = rng.randint(0, C_, size=B)
            k = 1.5 * 0.5 / B
            zd, yd = dev(z), dev(y, torch.int64)
            loss, dl = torch.full((2,), GUARD, device="cuda"), torch.full((B * C_ + 4,), GUARD, device="cuda")
            ops.softmax_ce(zd, yd, B, C_, 1.5, up, loss, dl)
            loss_only, dl_only = torch.full((1,), NAN, device="cuda"), torch.full((B * C_,), NAN, device="cuda")
            ops.softmax_ce(zd, yd, B, C_, 1.5, up, loss_only, None)
            ops.softmax_ce(zd, yd, B, C_, 1.5, up, None, dl_only)
            torch.cuda.synchronize()
            what = "ds_softmax_ce B=%d C=%d" % (B, C_)
            assert host(loss)[1] == GUARD and (host(dl)[B * C_:] == GUARD).all(), what + ": wrote past its outputs"
            got_loss, got_dl = host(loss)[:1], host(dl)[:B * C_].reshape(B, C_)
            HR.check_bits(host(loss_only), got_loss, what + " loss alone")
            HR.check_bits(host(dl_only).reshape(B, C_), got_dl, what + " dlogits alone")
            _ce_check(got_loss, got_dl, z, y, k, what, worst)
            if equal_row is not None:      # equal logits: softmax is 1 / C up to the rounding of the reciprocal and the product
                p = got_dl[equal_row].astype(np.float64) / k + (np.arange(C_) == y[equal_row])
                assert np.abs(p - 1.0 / C_).max() <= 4 * U, what
            # a label outside [0, C)
            r = B // 3
            for bad_label in (C_, -1):
                yb = y.copy()
                yb[r] = bad_label
                loss_b, dl_b = torch.full((1,), 0.0, device="cuda"), torch.full((B, C_), NAN, device="cuda")
                ops.softmax_ce(zd, dev(yb, torch.int64), B, C_, 1.5, up, loss_b, dl_b)
                torch.cuda.synchronize()
                assert np.isnan(host(loss_b)[0]), what + ": label %d did not poison the loss" % bad_label
                got_b = host(dl_b)
                assert np.isfinite(got_b).all(), what
                rest = np.arange(B) != r
                HR.check_bits(got_b[rest], got_dl[rest], what + " rows beside the poisoned one")
                _ce_check(None, got_b, z, yb, k, what + " label %d" % bad_label, worst)
    print("ds_softmax_ce B=%d: %s" % (B, worst))


# ---- ds_slab_epilogue_ce ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("M", [256, 257, 512])
def test_slab_epilogue_ce_is_the_combine_followed_by_the_cross_entropy(M):
    """Eight slabs + bias -> logits -> loss, dlogits in one workgroup (thread t: rows t and t + 256): the bits of ds_slab_epilogue
    followed by ds_softmax_ce.  Against fp64: a logit is nine additions in index order, |err| <= 9 u (sum_k |slab_k| + |bias|);
    loss and dlogits from the fp32 logits as in the ds_softmax_ce test.  M = 513 and N = 33 are refused before any launch."""
    from tumblr_emotions_amd import _lib
    ops = _ops()
    lib = _lib.load()
    worst = HR.Worst()
    splits = 8
    for N in (2, 15, 32):
        rng = np.random.RandomState(M + N)
        slabs = rng.normal(size=(splits, M, N)).astype(np.float32)
        bias = rng.normal(size=N).astype(np.float32)
        y = rng.randint(0, N, size=M)
        sd, bd, yd = dev(slabs), dev(bias), dev(y, torch.int64)
        ref = [torch.full((M, N), NAN, device="cuda"), torch.full((1,), NAN, device="cuda"), torch.full((M, N), NAN, device="cuda")]
        _lib.check(lib.ds_slab_epilogue(ops._p(sd), splits, M * N, N, M, N, ops._p(ref[0]), N, ops._p(bd), None, 0,
                                        ops.DS_EPI_BIAS, ops._stream()), "ds_slab_epilogue")
        ops.softmax_ce(ref[0], yd, M, N, 1.0, None, ref[1], ref[2])
        got = [torch.full((M * N + 4,), GUARD, device="cuda"), torch.full((2,), GUARD, device="cuda"),
               torch.full((M * N + 4,), GUARD, device="cuda")]
        _lib.check(lib.ds_slab_epilogue_ce(ops._p(sd), splits, M * N, N, M, N, ops._p(got[0]), ops._p(bd), ops._p(yd), 1.0, None,
                                           ops._p(got[1]), ops._p(got[2]), ops._stream()), "ds_slab_epilogue_ce")
        torch.cuda.synchronize()
        what = "ds_slab_epilogue_ce M=%d N=%d" % (M, N)
        got = [host(g) for g in got]
        assert (got[0][M * N:] == GUARD).all() and got[1][1] == GUARD and (got[2][M * N:] == GUARD).all(), what
        logits, loss, dl = got[0][:M * N].reshape(M, N), got[1][:1], got[2][:M * N].reshape(M, N)
        HR.check_bits(logits, host(ref[0]), what + " logits")
        HR.check_bits(loss, host(ref[1]), what + " loss")
        HR.check_bits(dl, host(ref[2]), what + " dlogits")
        s64 = slabs.astype(np.float64)
        HR.check_bound(logits, s64.sum(0) + bias, (splits + 1) * U * (np.abs(s64).sum(0) + np.abs(bias)), what + " logits", worst)
        _ce_check(loss, dl, logits, y, 1.0 / M, what, worst)
    for M_, N_ in ((513, 15), (M, 33)):
        z = torch.zeros(M_ * N_, device="cuda")
        rc = lib.ds_slab_epilogue_ce(ops._p(torch.zeros(splits * M_ * N_, device="cuda")), splits, M_ * N_, N_, M_, N_, ops._p(z), None,
                                     ops._p(torch.zeros(M_, dtype=torch.int64, device="cuda")), 1.0, None, None, None, ops._stream())
        assert rc == -1 and b"ds_slab_epilogue_ce" in lib.ds_last_error()      # DS_ERR_ARG
    print("ds_slab_epilogue_ce M=%d: %s" % (M, worst))


# ---- ds_lstm_cell_fwd / ds_lstm_cell_bwd ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("nslabs", [0, 3])
@pytest.mark.parametrize("B,H", [(40, 96), (7, 48), (1, 100)])
def test_lstm_cell_with_split_k_slabs_and_masked_rows(B, H, nslabs):
    """The step-wise recurrence's cell launches with the recurrent term as split-K slabs (nslabs 3) and without, at t = 2, 3, 4
    with row lengths 1 .. 9 (a t below, at and above the lengths; the one-row case has length 3): the formulas of
    test_lstm_cell_forward_backward at its 1e-5 gate (of max|ref|), in fp64 on the same fp32 inputs.  Rows at or past their
    length: state copied to the bit, gate gradients exactly 0, dc_prev the bits of dc, dh_carry the bits of dh plus the slabs
    added in index order; live rows carry exactly 0."""
    ops = _ops()
    worst = HR.Worst()
    f32 = np.float32
    seq = np.array([3, 1, 4, 2, 9, 5, 3, 4][:B] * (B // 8 + 1))[:B] if B > 1 else np.array([3])
    for t in (2, 3, 4):
        rng = np.random.RandomState(B + H + t + nslabs)
        pre, c0, h0 = (rng.normal(size=s).astype(f32) for s in ((B, 4 * H), (B, H), (B, H)))
        rec = (rng.normal(size=(max(nslabs, 1), B, 4 * H)) * 0.3).astype(f32)
        live = (t < seq)[:, None]
        z = pre.astype(np.float64) + (rec[:nslabs].astype(np.float64).sum(0) if nslabs else 0.0)
        i, j, f, o = np.split(z, 4, axis=1)
        si, tj, sf, so = S.sigmoid(i), np.tanh(j), S.sigmoid(f + 1.0), S.sigmoid(o)
        cn = c0 * sf + si * tj
        hn = np.tanh(cn) * so
        g, sd = dev(pre), dev(seq, torch.int64)
        cd, hd = torch.full((B, H), NAN, device="cuda"), torch.full((B, H), NAN, device="cuda")
        ops.lstm_cell_fwd(g, dev(c0), dev(h0), sd, t, B, H, 1.0, cd, hd, dev(rec) if nslabs else None, nslabs, B * 4 * H)
        torch.cuda.synchronize()
        what = "lstm cell B=%d H=%d nslabs=%d t=%d" % (B, H, nslabs, t)
        acts, c1, h1 = host(g), host(cd), host(hd)
        HR.check_close(c1, np.where(live, cn, c0), what + " c", rel=1e-5, worst=worst)
        HR.check_close(h1, np.where(live, hn, h0), what + " h", rel=1e-5, worst=worst)
        HR.check_close(acts, np.concatenate([si, tj, sf, so], 1), what + " activations", rel=1e-5, worst=worst)
        dead = ~live[:, 0]
        HR.check_bits(c1[dead], c0[dead], what + " c of the masked rows")
        HR.check_bits(h1[dead], h0[dead], what + " h of the masked rows")
        # backward, on the activations and the cell state the forward launch left
        dh, dc = rng.normal(size=(B, H)).astype(f32), rng.normal(size=(B, H)).astype(f32)
        dhs = (rng.normal(size=(max(nslabs, 1), B, H)) * 0.3).astype(f32)
        a_i, a_j, a_f, a_o = np.split(acts.astype(np.float64), 4, axis=1)
        dhv = dh.astype(np.float64) + (dhs[:nslabs].astype(np.float64).sum(0) if nslabs else 0.0)
        tc = np.tanh(c1.astype(np.float64))
        dct = dc + dhv * a_o * (1 - tc ** 2)
        ref_dg = np.where(live, np.concatenate([dct * a_j * a_i * (1 - a_i), dct * a_i * (1 - a_j ** 2),
                                                dct * c0 * a_f * (1 - a_f), dhv * tc * a_o * (1 - a_o)], 1), 0.0)
        dg = torch.full((B, 4 * H), NAN, device="cuda")
        dcp, dhc = torch.full((B, H), NAN, device="cuda"), torch.full((B, H), NAN, device="cuda")
        ops.lstm_cell_bwd(g, cd, dev(c0), dev(dh), dev(dc), sd, t, B, H, dg, dcp, dhc, dev(dhs) if nslabs else None, nslabs, B * H)
        torch.cuda.synchronize()
        dg, dcp, dhc = host(dg), host(dcp), host(dhc)
        HR.check_close(dg, ref_dg, what + " dgates", rel=1e-5, worst=worst)
        HR.check_close(dcp, np.where(live, dct * a_f, dc), what + " dc_prev", rel=1e-5, worst=worst)
        carry = dh.copy()
        for s in range(nslabs):
            carry = (carry + dhs[s]).astype(f32)
        HR.check_bits(dg[dead], np.zeros((int(dead.sum()), 4 * H), f32), what + " dgates of the masked rows")
        HR.check_bits(dcp[dead], dc[dead], what + " dc_prev of the masked rows")
        HR.check_bits(dhc[dead], carry[dead], what + " dh_carry of the masked rows")
        HR.check_bits(dhc[~dead], np.zeros((int((~dead).sum()), H), f32), what + " dh_carry of the live rows")
    print("lstm cell B=%d H=%d nslabs=%d: %s" % (B, H, nslabs, worst))


# ---- plumbing -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rows,cols,lds,ldd", [(37, 19, 23, 29), (1, 1, 1, 1), (1030, 515, 517, 516)])
def test_copy2d_strided_both_sides(rows, cols, lds, ldd):
    """Bit-exact copy of [rows, cols] between two row strides (the last shape takes a second grid-stride trip); the columns
    past `cols` of the destination and the elements behind it keep what they held."""
    ops = _ops()
    rng = np.random.RandomState(rows + cols)
    src = rng.normal(size=(rows, lds)).astype(np.float32)
    dst = torch.full((rows * ldd + 8,), GUARD, device="cuda")
    ops.copy2d(dev(src), lds, dst, ldd, rows, cols)
    torch.cuda.synchronize()
    got = host(dst)
    body = got[:rows * ldd].reshape(rows, ldd)
    HR.check_bits(body[:, :cols], src[:, :cols], "ds_copy2d")
    assert (body[:, cols:] == GUARD).all() and (got[rows * ldd:] == GUARD).all()


@pytest.mark.parametrize("n", [1, CAP + 1])
def test_fill_and_its_guard(n):
    ops = _ops()
    dst = torch.full((n + 8,), GUARD, device="cuda")
    ops.fill(dst, n, 3.25)
    torch.cuda.synchronize()
    got = host(dst)
    assert (got[:n] == 3.25).all() and (got[n:] == GUARD).all()


@pytest.mark.parametrize("cs,cd,pixels", [(3, 4, 1001), (1, 4, 1001), (5, 8, 70001), (4, 4, 33)])
def test_pad_channels_every_width(cs, cd, pixels):
    """dst[p, :cs] = src[p], dst[p, cs:] = 0, bit for bit ((5, 8) at 70 001 pixels takes a second grid-stride trip)."""
    ops = _ops()
    src = np.random.RandomState(cs + cd).normal(size=(pixels, cs)).astype(np.float32)
    dst = torch.full((pixels * cd + 8,), GUARD, device="cuda")
    ops.pad_channels(dev(src), cs, dst, cd, pixels)
    torch.cuda.synchronize()
    got = host(dst)
    body = got[:pixels * cd].reshape(pixels, cd)
    HR.check_bits(body[:, :cs], src, "ds_pad_channels")
    assert not body[:, cs:].any() and (got[pixels * cd:] == GUARD).all()
