"""tests/head_ref.py on the CPU: the fp64 heads against torch.autograd in float64 (in the manner of test_oracle_cross.py), the plan
arithmetic against the cases the GPU tests name, and every comparison helper of the head / text-dimension / step-tail GPU
tests against a planted error of the kind it is there to report."""
import numpy as np
import pytest
import torch

import head_ref as HR

RNG = np.random.RandomState(5)


def _joint_inputs(B, im, tx, fc, nc, rng):
    return (rng.normal(size=(B, im)), rng.normal(size=(B, tx)), rng.normal(size=(im + tx, fc)) * 0.05, rng.normal(size=fc) * 0.1,
            rng.normal(size=(fc, nc)) * 0.1, rng.normal(size=nc) * 0.1, rng.randint(0, nc, size=B))


@pytest.mark.parametrize("dims", [(7, 5, 9, 11, 4), (1, 3, 2, 6, 2), (12, 8, 1, 5, 15)])
def test_joint_head_matches_autograd(dims):
    B, im, tx, fc, nc = dims
    a_im, a_tx, W_fc, b_fc, W_sm, b_sm, y = _joint_inputs(B, im, tx, fc, nc, RNG)
    t = [torch.tensor(a, requires_grad=True) for a in (a_im, a_tx, W_fc, b_fc, W_sm, b_sm)]
    dense = torch.relu(torch.cat([t[0], t[1]], 1) @ t[2] + t[3])
    logits = dense @ t[4] + t[5]
    logits.retain_grad()
    loss = torch.nn.functional.cross_entropy(logits, torch.tensor(y))
    loss.backward()
    r = HR.joint_head(a_im, a_tx, W_fc, b_fc, W_sm, b_sm, y)
    np.testing.assert_allclose(r["dense"], dense.detach().numpy(), atol=1e-12)
    np.testing.assert_allclose(r["logits"], logits.detach().numpy(), atol=1e-12)
    np.testing.assert_allclose(r["loss"], float(loss.detach()), atol=1e-12)
    np.testing.assert_allclose(r["dlogits"], logits.grad.numpy(), atol=1e-12)
    for name, g in (("d_im", t[0]), ("d_tx", t[1]), ("W_fc", t[2]), ("b_fc", t[3]), ("W_softmax", t[4]), ("b_softmax", t[5])):
        np.testing.assert_allclose(r[name], g.grad.numpy(), atol=1e-12, err_msg=name)
    # following its own decisions changes nothing; following others' zeroes those units in both directions
    same = HR.joint_head(a_im, a_tx, W_fc, b_fc, W_sm, b_sm, y, decisions=r["pre"] > 0)
    assert all(np.array_equal(same[k], r[k]) for k in ("dense", "logits", "dlogits", "W_fc", "d_im", "d_tx"))
    off = HR.joint_head(a_im, a_tx, W_fc, b_fc, W_sm, b_sm, y, decisions=np.zeros((B, fc), bool))
    assert not off["dense"].any() and not off["d_im"].any() and not off["W_fc"].any()


@pytest.mark.parametrize("dims", [(6, 10, 5), (1, 4, 2), (9, 3, 15)])
def test_text_head_matches_autograd(dims):
    B, H, nc = dims
    h, W, b, y = RNG.normal(size=(B, H)), RNG.normal(size=(H, nc)) * 0.2, RNG.normal(size=nc) * 0.1, RNG.randint(0, nc, size=B)
    t = [torch.tensor(a, requires_grad=True) for a in (h, W, b)]
    logits = t[0] @ t[1] + t[2]
    logits.retain_grad()
    loss = torch.nn.functional.cross_entropy(logits, torch.tensor(y))
    loss.backward()
    r = HR.text_head(h, W, b, y)
    np.testing.assert_allclose(r["logits"], logits.detach().numpy(), atol=1e-12)
    np.testing.assert_allclose(r["loss"], float(loss.detach()), atol=1e-12)
    np.testing.assert_allclose(r["dlogits"], logits.grad.numpy(), atol=1e-12)
    for name, g in (("d_tx", t[0]), ("W_softmax", t[1]), ("b_softmax", t[2])):
        np.testing.assert_allclose(r[name], g.grad.numpy(), atol=1e-12, err_msg=name)


def test_slice_arithmetic_of_the_named_dims():
    """The K-tile counts the GPU tests rely on, as the split-K loop of ds_conv_igemm forms them."""
    assert HR.split_tiles(520, 8) == [5, 5, 5, 5, 5, 5, 3, 0] and HR.split_tiles(560, 8) == [5] * 7 + [0]
    assert HR.split_tiles(260, 4) == [5, 5, 5, 2] and HR.split_tiles(300, 4) == [5, 5, 5, 4]
    assert HR.split_tiles(648, 8)[-1] == 0 and HR.split_tiles(776, 8)[-1] == 0 and HR.split_tiles(512, 8) == [4] * 8
    empty = [K for K in range(512, 1100) if HR.split_tiles(K, 8)[-1] == 0]
    assert empty == list(range(513, 561)) + list(range(641, 673)) + list(range(769, 785))
    assert all(HR.split_tiles(K, 4)[-1] > 0 for K in range(256, 512))
    for K, s in ((520, 8), (260, 4), (300, 4), (776, 8), (512, 8), (256, 4)):
        r = HR.split_ranges(K, s)
        assert r[0][0] == 0 and r[-1][1] == K and all(a[1] == b[0] for a, b in zip(r, r[1:]))
    assert (HR.plan_splits(512, 256), HR.plan_splits(513, 256), HR.plan_splits(33, 255), HR.plan_splits(33, 511),
            HR.plan_splits(1, 512)) == (4, 0, 0, 4, 8)
    assert (HR.colsum_form(512), HR.colsum_form(513)) == ("one-launch", "two-stage")


def test_the_case_lists_name_every_form_and_the_old_ones_did_not():
    """The dims of test_head_dims_gpu.py are expected to reach every form (the GPU tests assert that the engines agree); the
    head dims the suite ran before reach neither a ragged nor an empty slice, nor the second trip of the fused cross entropy,
    nor the two-stage ds_colsum from a head."""
    new = set()
    for c in HR.JOINT_CASES:
        new |= HR.joint_forms(*c)[3]
    for c in HR.TEXT_CASES:
        new |= HR.text_forms(*c)[1]
    assert new == HR.ALL_FORMS, HR.ALL_FORMS - new
    old = set()
    for c in HR.OLD_JOINT_CASES:
        old |= HR.joint_forms(*c)[3]
    for c in HR.OLD_TEXT_CASES:
        old |= HR.text_forms(*c)[1]
    assert HR.ALL_FORMS - old == {"slice-ragged", "slice-empty", "ce-fused-second-trip", "colsum-two-stage"}, HR.ALL_FORMS - old
    # every threshold has a case on either side
    J = HR.JOINT_CASES
    assert {c[0] for c in J} >= {1, 256, 257, 512, 513} and {c[4] for c in J} >= {2, 32, 33, 40}
    assert sum((c[1] * c[3]) % 4 != 0 for c in J) >= 1


# ---- planted errors ---------------------------------------------------------------------------------------------------------

def _head_case():
    B, im, tx, fc, nc = 512, 24, 40, 32, 15
    a = _joint_inputs(B, im, tx, fc, nc, np.random.RandomState(9))
    return a, HR.joint_head(*a)


def test_helpers_accept_fp32_rounding():
    a, r = _head_case()
    for k in ("dense", "logits", "dlogits", "d_tx", "W_fc"):
        HR.check_close(r[k].astype(np.float32), r[k], k)
    HR.check_rows(r["dlogits"].astype(np.float32), r["dlogits"], "dlogits", 1e-5, floor=HR.ce_row_floor(15, 1 / 512))
    HR.check_bits(r["d_tx"].astype(np.float32), r["d_tx"].astype(np.float32).copy(), "d_tx")


def test_two_swapped_rows_of_d_tx_are_reported():
    _, r = _head_case()
    got = r["d_tx"].astype(np.float32)
    got[[3, 200]] = got[[200, 3]]
    with pytest.raises(AssertionError, match="d_tx"):
        HR.check_close(got, r["d_tx"], "d_tx")
    with pytest.raises(AssertionError, match="d_tx"):
        HR.check_bits(got, r["d_tx"].astype(np.float32), "d_tx")


@pytest.mark.parametrize("K,splits", [(520, 8), (512, 8), (260, 4)])
def test_a_missing_slab_is_reported(K, splits):
    """A GEMM result that lacks the sum of one split (the last one that owns K-tiles), and a slab left unwritten (NaN)."""
    rng = np.random.RandomState(K)
    a, w = rng.normal(size=(33, K)), rng.normal(size=(K, 15)) * 0.05
    full = a @ w
    k0, k1 = [r for r in HR.split_ranges(K, splits) if r[1] > r[0]][-1]
    HR.check_close(full.astype(np.float32), full, "gemm")
    with pytest.raises(AssertionError, match="gemm"):
        HR.check_close((full - a[:, k0:k1] @ w[k0:k1]).astype(np.float32), full, "gemm")
    with pytest.raises(AssertionError, match="gemm"):
        HR.check_close(np.full_like(full, np.nan), full, "gemm")
    with pytest.raises(AssertionError, match="slab"):
        HR.check_bits(np.full((33, 15), np.nan, np.float32), np.zeros((33, 15), np.float32), "slab")


def test_the_last_256_rows_off_by_1000_ulp_are_reported():
    """What a wrong second trip of the fused cross entropy (rows 256 .. 511) would look like at its smallest: per row against
    the row's own maximum, and as bits; the whole-tensor gate of the GEMMs (2e-4) is blind to it, which is why dlogits is
    held per row."""
    _, r = _head_case()
    ref = r["dlogits"]
    got = ref.astype(np.float32)
    bad = got.copy()
    bad[256:] = (bad[256:].view(np.int32) + 1000).view(np.float32)
    HR.check_rows(got, ref, "dlogits", 1e-5, floor=HR.ce_row_floor(15, 1 / 512))
    with pytest.raises(AssertionError, match="dlogits"):
        HR.check_rows(bad, ref, "dlogits", 1e-5, floor=HR.ce_row_floor(15, 1 / 512))
    with pytest.raises(AssertionError, match="dlogits"):
        HR.check_bits(bad, got, "dlogits")
    with pytest.raises(AssertionError, match="256 of 512"):
        HR.check_bound(bad.max(1), got.max(1).astype(np.float64), 4 * HR.U * np.abs(got).max(1), "dlogits")
    HR.check_close(bad, ref, "dlogits")          # (the blind one)


ADAM = dict(wd=4e-5, grad_scale=0.5, b1=0.9, b2=0.999, eps=1e-8)


@pytest.mark.parametrize("n,n_wd", [(1003, 40), (1003, 0), (1003, 1003), (3, 1), (3, 2), (1, 0), (1, 1), (70000, 69999)])
def test_adam_check_accepts_the_fp32_model_and_reports_a_boundary_off_by_one(n, n_wd):
    w, gs = HR.adam_inputs(n, n_wd, seed=n + n_wd)
    state = (w, np.zeros(n, np.float32), np.zeros(n, np.float32))
    for t in (1, 2, 3):
        lr_t = 1e-3 * np.sqrt(1 - 0.999 ** t) / (1 - 0.9 ** t)
        good = HR.adam_model_f32(*state[:1], gs[t - 1], *state[1:], n_wd, lr_t=lr_t, **ADAM)
        worst = HR.Worst()
        HR.check_adam(good, state, gs[t - 1], n_wd, lr_t=lr_t, what="adam", worst=worst, **ADAM)
        assert worst.ratio <= 1.0
        for off in (-1, 1):
            if not 0 <= n_wd + off <= n:
                continue
            bad = HR.adam_model_f32(*state[:1], gs[t - 1], *state[1:], n_wd + off, lr_t=lr_t, **ADAM)
            with pytest.raises(AssertionError, match="adam"):
                HR.check_adam(bad, state, gs[t - 1], n_wd, lr_t=lr_t, what="adam", **ADAM)
        state = good


def test_adam_check_reports_the_other_faults_too():
    """Weight decay dropped or halved, epsilon inside the square root, and an element the grid-stride loop never reached."""
    n, n_wd = 1003, 400
    w, gs = HR.adam_inputs(n, n_wd, seed=1)
    state = (w, np.zeros(n, np.float32), np.zeros(n, np.float32))
    lr_t = 1e-3 * np.sqrt(1 - 0.999) / (1 - 0.9)
    for change in (dict(wd=0.0), dict(wd=2e-5)):
        bad = HR.adam_model_f32(w, gs[0], state[1], state[2], n_wd, lr_t=lr_t, **dict(ADAM, **change))
        with pytest.raises(AssertionError):
            HR.check_adam(bad, state, gs[0], n_wd, lr_t=lr_t, what="adam", **ADAM)
    t, m, v = HR.adam_model_f32(w, gs[0], state[1], state[2], n_wd, lr_t=lr_t, **ADAM)
    inside = (w - np.float32(lr_t) * m / np.sqrt(v + np.float32(1e-8))).astype(np.float32)
    with pytest.raises(AssertionError):
        HR.check_adam((inside, m, v), state, gs[0], n_wd, lr_t=lr_t, what="adam", **ADAM)
    t2 = t.copy()
    t2[-1] = w[-1]
    with pytest.raises(AssertionError):
        HR.check_adam((t2, m, v), state, gs[0], n_wd, lr_t=lr_t, what="adam", **ADAM)
