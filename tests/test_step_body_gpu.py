"""One training-step body (SentimentNet._step_body): the eager step, every clone of a step of several clones and the captured
step enqueue the same sequence, and none of them goes through torch.autograd -- the engines write every gradient straight into
store.grad, so a step inside torch.no_grad() leaves the bits of a step outside it."""
import contextlib

import pytest
import torch

pytestmark = pytest.mark.gpu

SMALL = dict(nb_emotions=15, rnn_size=32, vocab_size=50, embedding_dim=20, post_size=10)
LR = 1e-3


def _net(mode, seed=7):
    from tumblr_emotions_amd.net import SentimentNet
    net = SentimentNet(mode=mode, **SMALL)
    net.initialize(seed=seed)
    return net


def _batch(rows):
    from tumblr_emotions_amd.synthetic import synthetic_batch_numpy, to_device
    return to_device(synthetic_batch_numpy(rows, 10, 50, seed=5))


@contextlib.contextmanager
def _recorded(monkeypatch):
    """The names of the library calls made inside the block, in order."""
    from tumblr_emotions_amd import _lib
    calls = []
    check = _lib.check
    monkeypatch.setattr(_lib, "check", lambda rc, what: (calls.append(what), check(rc, what))[1])
    try:
        yield calls
    finally:
        monkeypatch.setattr(_lib, "check", check)


def _two_steps(mode, rows, no_grad, **kw):
    net, batch = _net(mode), _batch(rows)
    with (torch.no_grad() if no_grad else contextlib.nullcontext()):
        for _ in range(2):
            net.train_step(batch, LR, **kw)
    torch.cuda.synchronize()
    return net


def _same_state(a, b):
    assert torch.equal(a.logits, b.logits) and not bool(torch.isnan(a.logits).any())
    la, lb = a.total_loss_value(), b.total_loss_value()
    assert la == la and la == lb
    for name in ("grad", "theta", "m", "v", "frozen"):
        x, y = getattr(a.store, name), getattr(b.store, name)
        assert not bool(torch.isnan(x).any()), name
        assert torch.equal(x, y), name
    for net in (a, b):
        assert net.logits.grad_fn is None and not net.logits.requires_grad
        assert not hasattr(net, "leaves")


@pytest.mark.parametrize("mode", ["joint", "text", "image"])
def test_train_step_needs_no_autograd(mode):
    """Two steps from the same initialisation, with autograd's recording on and inside torch.no_grad(): logits, loss, gradients,
    variables, Adam slots and moving statistics are bit-identical, and the logits carry no graph."""
    _same_state(_two_steps(mode, 8, False), _two_steps(mode, 8, True))


def test_clone_step_needs_no_autograd():
    """The same for a joint step of two clones of 8 rows."""
    _same_state(_two_steps("joint", 16, False, num_clones=2), _two_steps("joint", 16, True, num_clones=2))


@pytest.mark.parametrize("mode", ["joint", "text"])
def test_captured_body_is_the_eager_body(mode, monkeypatch):
    """capture_step on a warmed net runs one eager step (its warm-up, in the arrangement of the capture: one side stream in the
    image tower) and then captures one: the two halves of the calls it makes are the same list, Adam included."""
    net, batch = _net(mode), _batch(8)
    net.train_step(batch, LR)
    with _recorded(monkeypatch) as calls:
        assert net.capture_step(batch)
    torch.cuda.synchronize()
    n = len(calls)
    assert n > 0 and n % 2 == 0, n
    eager, captured = calls[:n // 2], calls[n // 2:]
    assert eager[-1] == "ds_adam_tf" and eager.count("ds_adam_tf") == 1
    assert eager == captured


def test_clone_body_is_the_plain_body(monkeypatch):
    """The second step of two clones of 8 rows against the second plain step of 8 rows: per clone the calls of the plain step;
    beside them the L2 term once, one accumulation per clone, one Adam."""
    K = 2
    lists = []
    for rows, kw in ((8 * K, dict(num_clones=K)), (8, {})):
        net, batch = _net("joint"), _batch(rows)
        net.train_step(batch, LR, **kw)
        with _recorded(monkeypatch) as calls:
            net.train_step(batch, LR, **kw)
        torch.cuda.synchronize()
        lists.append(list(calls))
    clone, plain = lists
    beside = ("ds_grad_accumulate", "ds_adam_tf", "ds_sumsq")
    assert [c for c in clone if c not in beside] == K * [c for c in plain if c not in beside]
    assert plain.count("ds_sumsq") > 0 and clone.count("ds_sumsq") == plain.count("ds_sumsq")
    assert clone.count("ds_grad_accumulate") == K and plain.count("ds_grad_accumulate") == 0
    assert clone.count("ds_adam_tf") == 1 and plain.count("ds_adam_tf") == 1
