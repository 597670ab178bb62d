"""label_smoothing and class_weights without a GPU: the fp64 restatement (tests/loss_ref.py) against
torch.autograd of its own loss written out, against head_ref.softmax_ce at the defaults, its comparison helpers against planted
errors, every configuration check_loss_config / loss_net_kwargs refuse, and the ABI of the two new entry points."""
import ctypes as C

import numpy as np
import pytest
import torch

import head_ref as HR
import loss_ref as LR


def _case(B=7, nc=5, seed=0):
    rng = np.random.RandomState(seed)
    return rng.uniform(-6, 6, size=(B, nc)), rng.randint(0, nc, size=B)


WEIGHTS = (None, [1.0] * 5, [0.5, 0.0, 2.0, 1.0, 0.0], [0.0, 3.0, 0.25, 0.0, 1.5])


@pytest.mark.parametrize("eps", [0.0, 0.1, 0.9])
@pytest.mark.parametrize("cw", WEIGHTS)
def test_gradient_is_autograds_of_the_loss_written_out(eps, cw):
    """Written out here a second time, with an explicit one-hot matrix and log-softmax instead of loss_ref's logsumexp, and
    divided by the count of non-zero weights (F.cross_entropy(weight=) divides by their sum and is not the reference)."""
    z, y = _case(seed=3)
    zt = torch.tensor(z, dtype=torch.float64, requires_grad=True)
    onehot = torch.zeros(z.shape, dtype=torch.float64)
    onehot[torch.arange(len(y)), torch.as_tensor(y)] = 1.0
    q = onehot * (1 - eps) + eps / z.shape[1]
    per_row = -(q * torch.log_softmax(zt, 1)).sum(1)
    w = torch.ones(len(y), dtype=torch.float64) if cw is None else torch.tensor(cw, dtype=torch.float64)[torch.as_tensor(y)]
    P = int((w != 0).sum())
    assert 0 < P and (cw is None or cw[0] == 1.0 or P < len(y))
    loss = (w * per_row).sum() / P
    loss.backward()
    loss = loss.detach()
    got_loss, got_dl = LR.softmax_ce(z, y, eps, cw, grad_scale=1.5)
    assert abs(got_loss - float(loss)) <= 1e-14 * abs(float(loss))
    assert np.abs(got_dl - 1.5 * zt.grad.numpy()).max() <= 1e-15
    # the torch form the oracle model uses is the same function
    zt2 = torch.tensor(z, dtype=torch.float64, requires_grad=True)
    t = LR.torch_ce(zt2, y, eps, cw)
    t.backward()
    t = t.detach()
    assert abs(float(t) - got_loss) <= 1e-14 * abs(got_loss) and np.abs(zt2.grad.numpy() * 1.5 - got_dl).max() <= 1e-15
    if float(w.sum()) != P:      # dividing by sum(w), as F.cross_entropy(weight=) does, is another number
        assert abs(float((w * per_row).sum().detach() / w.sum()) - got_loss) > 1e-3 * got_loss


def test_defaults_are_the_plain_mean_cross_entropy():
    z, y = _case(B=9, seed=4)
    a_loss, a_dl = HR.softmax_ce(z.copy(), y)
    for cw in (None, [1.0] * 5):
        b_loss, b_dl = LR.softmax_ce(z, y, 0.0, cw)
        assert abs(a_loss - b_loss) <= 1e-15 * abs(a_loss) and np.abs(a_dl - b_dl).max() <= 1e-16
    assert float(LR.torch_ce(torch.tensor(z), y)) == pytest.approx(a_loss, rel=1e-14)


def test_no_counted_row_and_labels_out_of_range():
    z, y = _case(seed=5)
    cw = np.ones(5)
    cw[np.unique(y)] = 0.0
    loss, dl = LR.softmax_ce(z, y, 0.1, cw)
    assert loss == 0.0 and not dl.any()
    assert float(LR.torch_ce(torch.tensor(z), y, 0.1, cw)) == 0.0
    for bad in (5, -1):
        yb = y.copy()
        yb[2] = bad
        cw = np.array([0.0, 2.0, 3.0, 4.0, 5.0])
        loss, dl = LR.softmax_ce(z, yb, 0.2, cw, grad_scale=2.0)
        p, q, w, P, _, ok = LR.terms(z, yb, 0.2, cw)
        assert np.isnan(loss) and not ok[2] and w[2] == 1.0 and P == int((cw[yb[ok]] != 0).sum()) + 1
        assert np.array_equal(q[2], np.full(5, 0.2 / 5)) and np.allclose(dl[2], (p[2] - 0.04) * 2.0 / P, rtol=1e-15)
        assert np.isfinite(dl).all()


def test_helpers_catch_planted_errors():
    rng = np.random.RandomState(6)
    z = rng.uniform(-60, 60, size=(40, 15)).astype(np.float32)
    y = rng.randint(0, 15, size=40)
    cw = rng.uniform(0.25, 2, size=15).astype(np.float32)
    cw[y[0]] = 0.0
    gs = 0.75
    loss, dl = LR.softmax_ce(z.astype(np.float64), y, float(np.float32(0.1)), cw.astype(np.float64), gs)
    good = np.float32(loss), dl.astype(np.float32)
    worst = HR.Worst()
    LR.check_ce(good[0], good[1], z, y, 0.1, cw, gs, "exact", worst)
    assert 0 < worst.ratio < 1
    with pytest.raises(AssertionError, match="loss"):
        LR.check_ce(good[0] * np.float32(1 + 3e-5), None, z, y, 0.1, cw, gs, "loss off by 3e-5")
    with pytest.raises(AssertionError, match="loss"):
        LR.check_ce(np.float32(np.nan), None, z, y, 0.1, cw, gs, "NaN loss")
    live = int(np.argmax(cw[y] != 0))
    bad = good[1].copy()
    bad[live, 3] += 3e-5 * np.abs(bad[live]).max() + 2 * LR.row_floor(15, cw[y[live]], gs / 39)
    with pytest.raises(AssertionError, match="row %d" % live):
        LR.check_ce(None, bad, z, y, 0.1, cw, gs, "one entry off")
    bad = good[1].copy()
    bad[0, 0] = 1e-30      # (row 0 has weight 0: not even a denormal-sized gradient)
    with pytest.raises(AssertionError):
        LR.check_ce(None, bad, z, y, 0.1, cw, gs, "a dead row moved")
    bad = good[1].copy()
    bad[5, 5] = np.nan
    with pytest.raises(AssertionError, match="finite"):
        LR.check_ce(None, bad, z, y, 0.1, cw, gs, "NaN entry")
    # the gradient of the unsmoothed, unweighted loss is not the gradient of this one, and the other way round
    with pytest.raises(AssertionError):
        LR.check_ce(None, HR.softmax_ce(z.astype(np.float64), y)[1] * gs, z, y, 0.1, cw, gs, "plain gradient")
    with pytest.raises(AssertionError):
        LR.check_ce(None, good[1], z, y, 0.0, None, gs, "weighted gradient held against the plain loss")
    # a label outside [0, C): a finite loss is an error
    yb = y.copy()
    yb[7] = 15
    with pytest.raises(AssertionError, match="poison"):
        LR.check_ce(np.float32(1.0), None, z, yb, 0.1, cw, gs, "finite loss")
    LR.check_ce(np.float32(np.nan), None, z, yb, 0.1, cw, gs, "poisoned loss")
    # the floor: nothing for a dead row, C + 9 roundings of w k otherwise
    assert LR.row_floor(15, 0.0, 1.0) == 0.0 and LR.row_floor(15, 2.0, 0.5) == 24 * 2.0 ** -24


def test_check_loss_config_refuses_before_any_device():
    from tumblr_emotions_amd.net import check_loss_config
    from tumblr_emotions_amd.training import loss_net_kwargs
    ok = [1.0] * 14 + [0.0]
    assert check_loss_config() == (0.0, None) and check_loss_config(0.0, None) == (0.0, None)
    assert check_loss_config(0.1, ok) == (0.1, tuple(ok)) and check_loss_config(0, np.asarray(ok)) == (0.0, tuple(ok))
    assert check_loss_config(np.float32(0.5))[0] == 0.5 and check_loss_config(0.25, [2] * 3, nb_emotions=3)[1] == (2.0,) * 3
    for bad in (True, False, "0.1", -0.1, 1.0, 1.5, float("nan"), float("inf"), [0.1], np.bool_(True)):
        with pytest.raises(ValueError, match="label_smoothing"):
            check_loss_config(bad)
        with pytest.raises(ValueError, match="label_smoothing"):
            loss_net_kwargs({"label_smoothing": bad})
    for bad in ([1.0] * 14, [1.0] * 16, [], [0.0] * 15, [1.0] * 14 + [-1.0], [1.0] * 14 + [float("nan")],
                [1.0] * 14 + [float("inf")], [1.0] * 14 + [True], [1.0] * 14 + ["1"], 1.0, "balanced", {0: 1.0},
                [1.0] * 14 + [None]):
        with pytest.raises(ValueError, match="class_weights"):
            check_loss_config(0.1, bad)
    for bad in ([0.0] * 15, [1.0] * 14 + [-1.0], [1.0] * 14 + [True], "balanced", 2.0, [1.0, float("nan")]):
        with pytest.raises(ValueError, match="class_weights"):
            loss_net_kwargs({"class_weights": bad})
    # the keys-absent case, in every spelling
    for cfg in ({}, {"label_smoothing": None}, {"label_smoothing": 0.0}, {"label_smoothing": 0, "class_weights": None}):
        assert loss_net_kwargs(cfg) == {}
    assert loss_net_kwargs({"label_smoothing": 0.1, "batch_size": 8}) == {"label_smoothing": 0.1}
    assert loss_net_kwargs({"class_weights": ok, "label_smoothing": 0.0}) == {"class_weights": ok}
    assert loss_net_kwargs({"class_weights": tuple(ok), "label_smoothing": 0.2, "dtype": "bf16"}) == \
        {"class_weights": ok, "label_smoothing": 0.2}
    # the net itself refuses before it looks for a device (no GPU here: a valid configuration gets as far as that)
    from tumblr_emotions_amd.net import SentimentNet
    with pytest.raises(ValueError, match="label_smoothing"):
        SentimentNet(mode="text", label_smoothing=1.0)
    with pytest.raises(ValueError, match="exactly nb_emotions = 15"):
        SentimentNet(mode="text", class_weights=[1.0] * 3)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            SentimentNet(mode="text", label_smoothing=0.1, class_weights=ok)


def test_descriptor_and_entry_points_are_the_headers():
    import os
    import re
    from tumblr_emotions_amd import _lib
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ds_kernels.h")).read()
    m = re.search(r"typedef struct ds_ce_desc \{(.*?)\} ds_ce_desc;", header, flags=re.S)
    fields = re.findall(r"(\w+)\s*;", m.group(1))
    assert fields == [f[0] for f in _lib.CeDesc._fields_] == ["label_smoothing", "class_weights"]
    assert C.sizeof(_lib.CeDesc) == 16 and _lib.CeDesc.class_weights.offset == 8
    lib = _lib.load()
    assert lib.ds_version() == 4
    d = _lib.CeDesc(0.1, None)
    # bad arguments are codes, before any launch: no logits, smoothing outside [0, 1), the fused entry's limits
    assert lib.ds_softmax_ce_opts(C.byref(d), None, None, 1, 1, 1.0, None, None, None, None) == -1
    assert b"ds_softmax_ce_opts" in lib.ds_last_error()
    one = C.c_void_p(16)      # (never dereferenced: the checks come first)
    for bad in (1.0, -0.5, float("nan")):
        assert lib.ds_softmax_ce_opts(C.byref(_lib.CeDesc(bad, None)), one, one, 1, 1, 1.0, None, None, None, None) == -1
        assert b"label_smoothing" in lib.ds_last_error()
    for M, N in ((513, 15), (8, 33), (0, 15)):
        assert lib.ds_slab_epilogue_ce_opts(C.byref(d), one, 8, M * N, N, M, N, one, None, one, 1.0, None, None, None, None) == -1
        assert b"ds_slab_epilogue_ce_opts" in lib.ds_last_error()
