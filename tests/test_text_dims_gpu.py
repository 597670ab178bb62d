"""The text model at its dimension edges against the fp64 oracle (test_model_gpu._check_step, two steps from identical state):
hidden sizes the persistent LSTM does not cover (48, 100: one GEMM plus one cell launch per step), T = 1 and B = 1 on either
path, a batch past one 256-row tile, a batch past 512 rows (the head on the plain plans, ds_colsum's two-stage form on dlogits)
and a one-column embedding.  Every batch with T > 1 holds the lengths 1 and T and a run of equal lengths (the length sort's
ties), with the pad id past each length.  The gates are _check_step's own; on an MI355X the worst figure of any case is
0.0035 of its gate (a resolved entry after the first Adam step, 3.5e-8 against 1e-5; logits <= 1.2e-7, gradients <= 2.2e-7
relative L2), and the file takes 2.4 s."""
import numpy as np
import pytest
import torch

from oracle import tf_semantics as S
from oracle import torch_ref as R

pytestmark = pytest.mark.gpu

# (V, D, H, T, B, persistent)
DIMS = [(30, 7, 48, 5, 6, False), (40, 50, 100, 9, 17, False),      # step-wise fallback
        (30, 7, 48, 1, 1, False), (30, 12, 32, 1, 1, True),         # T = 1 and B = 1, either path
        (40, 12, 32, 3, 257, True),                                  # past one 256-row tile; one-launch ds_colsum on dlogits
        (40, 12, 256, 4, 513, True),                                 # head on the plain plans, two-stage ds_colsum
        (40, 1, 64, 4, 5, True)]                                     # D = 1


def edge_batch(B, T, V, seed):
    rng = np.random.RandomState(seed)
    lens = rng.randint(1, T + 1, size=B).astype(np.int64)
    if T > 1:
        assert B >= 5
        lens[0], lens[1] = 1, T
        lens[2:min(B, 6)] = max(1, T // 2)
    ids = rng.randint(0, V, size=(B, T)).astype(np.int64)
    ids[np.arange(T)[None, :] >= lens[:, None]] = V          # pad id = unk id = V
    return {"texts": ids, "seq_lens": lens, "labels": rng.randint(0, 15, size=B).astype(np.int64)}


@pytest.mark.parametrize("dims", DIMS, ids=lambda d: "V%d-D%d-H%d-T%d-B%d" % d[:5])
def test_text_step_at_the_dimension_edges(dims):
    from test_model_gpu import _check_step, _sync_from_oracle
    from tumblr_emotions_amd import ops
    from tumblr_emotions_amd.net import SentimentNet
    V, D, H, T, B, persistent = dims
    rng = np.random.RandomState(100 + H + T + B)
    params = R.make_params("text", rng, num_classes=15, embed_dim=D, rnn_size=H, dtype=np.float64)
    params["Text/rnn/basic_lstm_cell/bias"] = rng.normal(0, 0.1, size=4 * H)
    emb = S.synthetic_embedding(V, D).astype(np.float64)
    batch = edge_batch(B, T, V, seed=B + T)
    if T > 1:
        lens = batch["seq_lens"]
        assert lens.min() == 1 and lens.max() == T and np.bincount(lens).max() >= 2
    ref = R.DeepSentimentRef(params, emb, "text", torch.float64)
    net = SentimentNet(mode="text", nb_emotions=15, rnn_size=H, vocab_size=V, embedding_dim=D, post_size=T)
    net.load_state_dict(dict(params, **{"Text/W_embedding": emb}))
    for i in range(2):
        if i:
            _sync_from_oracle(net, ref, emb)
        report = {}
        _check_step(net, ref, batch, 1e-3, first=(i == 0), report=report)
        # the gates of _check_step: logits and loss 1e-3, gradients 1e-3 (relative L2), resolved entries 1e-5
        ratio = max(report["logits"] / 1e-3, report["loss"] / 1e-3, report["grad"][0] / 1e-3, report["resolved_max"][0] / 1e-5)
        print("V%d D%d H%d T%d B%d step %d: max|dlogits| %.2e |dloss| %.2e worst gradient %.2e (%s) worst resolved entry %.2e; "
              "worst error / bound = %.3g" % (V, D, H, T, B, i + 1, report["logits"], report["loss"], report["grad"][0],
                                              report["grad"][1], report["resolved_max"][0], ratio))
    assert net.text.use_seq is persistent
    assert isinstance(net.head.sm, ops.SplitGemm) == (B <= 512 and H >= 256)
