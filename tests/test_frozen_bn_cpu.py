"""Frozen-BatchNorm training (SentimentNet(frozen_bn=True)) -- what can be checked without a GPU: the backward
formulas the kernels implement, and the fp64 reference the GPU tests compare against.

The reference needs no oracle change: FrozenBNRef clears `is_training` only around DeepSentimentRef._cbr, which gives
slim.batch_norm(is_training=False) -- moving statistics -- inside a tower whose dropout stays on; `bn_batch_stats` stays empty,
so the unchanged train_step applies no moving-average update."""
import numpy as np
import torch

from oracle import tf_semantics as S
from oracle import torch_ref as R


class FrozenBNRef(R.DeepSentimentRef):
    """DeepSentimentRef with every BatchNorm on its moving statistics while everything else trains."""

    def _cbr(self, x, scope, stride=1):
        keep = self.is_training
        self.is_training = False
        try:
            return super()._cbr(x, scope, stride)
        finally:
            self.is_training = keep


def test_pointwise_backward_formulas_match_autograd_in_fp64():
    """dz = rstd * g and dbeta = sum_{N,H,W} g with g = dy * [z*rstd + shift > 0], shift = beta - moving_mean * rstd: the
    derivative of relu(z*rstd + shift) for FIXED statistics -- no mean terms."""
    rng = np.random.RandomState(3)
    N, H, W, C = 3, 5, 4, 8
    z = torch.tensor(rng.normal(0, 1, size=(N, H, W, C)), requires_grad=True)
    beta = torch.tensor(rng.normal(0, 0.3, size=C), requires_grad=True)
    mm = torch.tensor(rng.normal(0, 0.5, size=C))
    mv = torch.tensor(rng.uniform(0.2, 3.0, size=C))
    dy = torch.tensor(rng.normal(0, 1, size=(N, H, W, C)))
    rstd = 1.0 / torch.sqrt(mv + S.BN_EPS)
    y = torch.relu(z * rstd + (beta - mm * rstd))
    (y * dy).sum().backward()
    with torch.no_grad():
        g = dy * ((z * rstd + (beta - mm * rstd)) > 0)
        assert (g != 0).any() and (g == 0).any()
        np.testing.assert_allclose(z.grad.numpy(), (rstd * g).numpy(), rtol=0, atol=1e-15)
        np.testing.assert_allclose(beta.grad.numpy(), g.sum((0, 1, 2)).numpy(), rtol=0, atol=1e-13)


def test_frozen_reference_step_reads_but_never_writes_the_moving_statistics():
    """One step of the subclass at 224x224: the moving statistics keep their bits, the logits depend on them (they are what
    normalises), dropout is applied, and every trainable variable -- all 57 betas among them -- gets a gradient."""
    rng = np.random.RandomState(5)
    params = R.make_params("image", rng, num_classes=15)
    for k in params:
        if k.endswith("moving_variance"):
            params[k] = rng.uniform(0.5, 2.0, size=params[k].shape).astype(params[k].dtype)
    batch = S.synthetic_batch(2, 4, 20, seed=1)
    mask = (rng.uniform(size=(2, 1024)) < 0.8).astype(np.float32)
    ref = FrozenBNRef(params, None, "image", torch.float32)
    before = {k: v.clone() for k, v in ref.p.items() if k.endswith(("moving_mean", "moving_variance"))}
    assert len(before) == 2 * 57
    out = ref.train_step(batch, 1e-3, torch.tensor(mask))
    assert ref.bn_batch_stats == {} and ref.is_training
    for k, v in before.items():
        assert torch.equal(ref.p[k], v), k
    assert sum(n.endswith("BatchNorm/beta") for n in out["grads"]) == 57
    assert all(torch.isfinite(g).all() for g in out["grads"].values())
    with torch.no_grad():
        plain = FrozenBNRef(params, None, "image", torch.float32)
        no_drop = plain.forward(batch)
        dropped = plain.forward(batch, torch.tensor(mask))
        assert not torch.equal(no_drop, dropped)                       # dropout stays on
        assert torch.equal(dropped, out["logits"])
        k = "InceptionV1/Mixed_5c/Branch_0/Conv2d_0a_1x1/BatchNorm/moving_variance"
        plain.p[k] = plain.p[k] * 4.0
        assert not torch.equal(plain.forward(batch), no_drop)          # ... and the moving statistics are what normalises
