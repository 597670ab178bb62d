"""ds_eval_metrics_update against a NumPy fp64 statement of the same definitions: every integer (confusion matrix, rank
histogram, the three counters) exactly, the cross-entropy sum within 1e-9 * max(1, |ref|) -- the kernel's arithmetic is
double throughout, so the expected error at these sizes is below 1e-12, and a slip to fp32 would show as about 1e-6."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# (B, C, ldl): one row / tiny; one row past a 256-thread group; a padded row stride; both sides of the lane-per-row /
# wave-per-row threshold (C = 32 | 33), the second with more rows than one 16-row workgroup; rows wider than a wavefront
# and than 256; many workgroups
SHAPES = [(1, 2, 2), (7, 3, 3), (257, 15, 15), (64, 15, 24), (260, 32, 32), (21, 33, 33), (33, 1000, 1000), (4096, 15, 15)]
IDS = ["%dx%d%s" % (b, c, "" if l == c else "_ld%d" % l) for b, c, l in SHAPES]


def reference(logits, labels):
    """(counts int64 [C*C + C + 4], loss sum) of fp32 logits [B, C] and int64 labels [B], in NumPy fp64."""
    B, C = logits.shape
    counts = np.zeros(C * C + C + 4, np.int64)
    loss = 0.0
    for b in range(B):
        z, y = logits[b], int(labels[b])
        if not np.isfinite(z).all():
            counts[C * C + C + 1] += 1
            continue
        if not 0 <= y < C:
            counts[C * C + C + 2] += 1
            continue
        pred = int(np.argmax(z))                       # the first of the maximal logits
        rank = int((z > z[y]).sum() + (z[:y] == z[y]).sum())
        counts[y * C + pred] += 1
        counts[C * C + rank] += 1
        counts[C * C + C] += 1
        z64 = z.astype(np.float64)
        m = z64.max()
        loss += float(np.log(np.exp(z64 - m).sum()) + m - z64[y])
    return counts, loss


def on_device(logits, ldl=None):
    """fp32 [B, C] on the device with row stride ldl; the padding columns hold NaN, which a read past C would count."""
    B, C = logits.shape
    ldl = C if ldl is None else ldl
    buf = torch.full((B, ldl), float("nan"), dtype=torch.float32, device="cuda")
    buf[:, :C] = torch.from_numpy(logits)
    return buf[:, :C]


def run(logits, labels, ldl=None, metrics=None):
    from tumblr_emotions_amd.metrics import StreamingMetrics
    m = metrics or StreamingMetrics(logits.shape[1], "cuda")
    m.update(on_device(logits, ldl), torch.from_numpy(labels).cuda())
    return m


def check(logits, labels, ldl=None):
    want_counts, want_loss = reference(logits, labels)
    counts, loss = run(logits, labels, ldl).state()
    C = logits.shape[1]
    print("B=%d C=%d: n=%d loss=%.17g ref=%.17g |d|=%.3e" % (logits.shape[0], C, counts[C * C + C], loss[0], want_loss,
                                                           abs(loss[0] - want_loss)))
    np.testing.assert_array_equal(counts, want_counts)
    assert counts[-1] == 0
    assert abs(loss[0] - want_loss) <= 1e-9 * max(1.0, abs(want_loss))
    return counts, loss


def random_case(B, C, seed):
    rng = np.random.RandomState(seed)
    return rng.normal(size=(B, C)).astype(np.float32), rng.randint(0, C, size=B).astype(np.int64)


@pytest.mark.parametrize("B,C,ldl", SHAPES, ids=IDS)
def test_random_normal_logits(B, C, ldl):
    logits, labels = random_case(B, C, seed=B + C)
    counts, _ = check(logits, labels, ldl)
    assert counts[C * C + C] == B and counts[:C * C].sum() == B and counts[C * C:C * C + C].sum() == B


@pytest.mark.parametrize("B,C,ldl", SHAPES, ids=IDS)
def test_large_scale_and_offsets_logsumexp_stability(B, C, ldl):
    logits, labels = random_case(B, C, seed=3 * B + C)
    offset = np.where(np.arange(B) % 2 == 0, 3e4, -3e4).astype(np.float32)
    logits = (logits * np.float32(1e4) + offset[:, None]).astype(np.float32)
    check(logits, labels, ldl)


@pytest.mark.parametrize("B,C,ldl", SHAPES, ids=IDS)
def test_rows_of_all_equal_logits(B, C, ldl):
    """Every index is maximal: the prediction is index 0, the label's rank is the label, the loss log(C)."""
    rng = np.random.RandomState(B)
    logits = np.repeat(rng.normal(size=(B, 1)).astype(np.float32) * np.float32(50), C, axis=1)
    labels = rng.randint(0, C, size=B).astype(np.int64)
    counts, loss = check(logits, labels, ldl)
    conf = counts[:C * C].reshape(C, C)
    assert conf[:, 1:].sum() == 0
    np.testing.assert_array_equal(counts[C * C:C * C + C], np.bincount(labels, minlength=C))
    assert abs(loss[0] - B * np.log(C)) <= 1e-9 * max(1.0, B * np.log(C))


@pytest.mark.parametrize("B,C,ldl", [s for s in SHAPES if s[1] >= 3], ids=[i for i, s in zip(IDS, SHAPES) if s[1] >= 3])
def test_ties_with_the_label_follow_the_rank_and_prediction_rules(B, C, ldl):
    """Row kinds by b % 4: the label ties with a LOWER index at the maximum (prediction = that index, rank 1); with a HIGHER
    index at the maximum (prediction = the label, rank 0); with a lower index below the maximum; with a higher one below it."""
    rng = np.random.RandomState(C)
    logits = rng.normal(size=(B, C)).astype(np.float32)
    labels = np.zeros(B, np.int64)
    for b in range(B):
        kind = b % 4
        if kind in (0, 2):
            y = rng.randint(1, C)
            other = rng.randint(0, y)
        else:
            y = rng.randint(0, C - 1)
            other = rng.randint(y + 1, C)
        labels[b] = y
        top = np.float32(np.abs(logits[b]).max() + 1.0)
        if kind < 2:
            logits[b, y] = logits[b, other] = top
        else:
            logits[b, other] = logits[b, y]
    counts, _ = check(logits, labels, ldl)
    rank_hist = counts[C * C:C * C + C]
    if B >= 4:
        assert rank_hist[0] >= B // 4 and rank_hist[1] >= B // 4
    assert np.trace(counts[:C * C].reshape(C, C)) == rank_hist[0]        # rank 0 exactly when the prediction is the label


@pytest.mark.parametrize("B,C,ldl", [(64, 15, 24), (257, 15, 15), (33, 1000, 1000)], ids=["64x15_ld24", "257x15", "33x1000"])
def test_non_finite_rows_and_labels_out_of_range_are_counted_apart(B, C, ldl):
    logits, labels = random_case(B, C, seed=77)
    logits[3, C - 1] = np.nan
    logits[5, 0] = np.inf
    logits[6, C // 2] = -np.inf
    labels[8] = -1
    labels[9] = C
    labels[10] = np.iinfo(np.int64).max          # no address may be formed from such a label
    labels[11] = np.iinfo(np.int64).min
    logits[12, 1] = np.nan                       # non-finite AND a bad label: non-finite comes first
    labels[12] = C + 7
    counts, _ = check(logits, labels, ldl)
    n, n_nonfinite, n_bad = counts[C * C + C:C * C + C + 3]
    assert (n, n_nonfinite, n_bad) == (B - 8, 4, 4)
    assert counts[:C * C].sum() == n and counts[C * C:C * C + C].sum() == n


@pytest.mark.parametrize("B,C,ldl", [(257, 15, 15), (33, 1000, 1000)], ids=["257x15", "33x1000"])
def test_every_class_absent_except_one(B, C, ldl):
    logits, _ = random_case(B, C, seed=5)
    labels = np.full(B, C - 2, np.int64)
    counts, _ = check(logits, labels, ldl)
    conf = counts[:C * C].reshape(C, C)
    assert conf[C - 2].sum() == B and conf.sum() == B
    from tumblr_emotions_amd.metrics import summarize
    r = summarize(counts, np.zeros(1), C)
    assert r["per_class"]["support"][C - 2] == B and sum(r["per_class"]["support"]) == B
    assert r["macro_f1"] == r["per_class"]["f1"][C - 2]


@pytest.mark.parametrize("B,C", [(300, 15), (40, 1000)], ids=["300x15", "40x1000"])
def test_accumulation_reset_and_bitwise_reproducibility(B, C):
    from tumblr_emotions_amd.metrics import StreamingMetrics
    logits, labels = random_case(B, C, seed=11)
    labels[1] = -5
    logits[2, 0] = np.nan
    cuts = [0, B // 3, B // 3 + 1, B]
    m = StreamingMetrics(C, "cuda")
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        run(logits[lo:hi], labels[lo:hi], metrics=m)
    parts_counts, parts_loss = m.state()
    whole_counts, whole_loss = run(logits, labels).state()
    np.testing.assert_array_equal(parts_counts, whole_counts)
    want_counts, want_loss = reference(logits, labels)
    np.testing.assert_array_equal(parts_counts, want_counts)
    for loss in (parts_loss[0], whole_loss[0]):
        assert abs(loss - want_loss) <= 1e-9 * max(1.0, abs(want_loss))
    m.reset()
    counts, loss = m.state()
    assert not counts.any() and loss[0] == 0.0 and loss.view(np.int64)[0] == 0
    # after reset the accumulators start again; two runs give identical bits, the loss included
    run(logits, labels, metrics=m)
    again_counts, again_loss = m.state()
    np.testing.assert_array_equal(again_counts, whole_counts)
    assert again_loss.view(np.int64)[0] == whole_loss.view(np.int64)[0]
    r = m.result()
    assert r["n"] == B - 2 and r["n_nonfinite"] == 1 and r["n_bad_label"] == 1
    assert sorted(r["top_k"]) == [1, 3, 5]
    assert r["top_k"][1] == r["accuracy"] <= r["top_k"][3] <= r["top_k"][5] <= 1.0
    assert abs(r["loss"] - want_loss / (B - 2)) <= 1e-9 * max(1.0, abs(want_loss) / (B - 2))


@pytest.mark.parametrize("B,C,ldl", [(257, 15, 15), (4096, 15, 15), (33, 1000, 1000)], ids=["257x15", "4096x15", "33x1000"])
def test_accuracy_equals_argmax_accuracy_on_tie_free_logits(B, C, ldl):
    logits, labels = random_case(B, C, seed=9)
    assert all(len(np.unique(row)) == C for row in logits)
    dev, lab = on_device(logits, ldl), torch.from_numpy(labels).cuda()
    from tumblr_emotions_amd.metrics import StreamingMetrics
    m = StreamingMetrics(C, "cuda")
    m.update(dev, lab)
    r = m.result()
    hits = dev.argmax(1) == lab
    assert r["accuracy"] == int(hits.sum().item()) / B
    assert np.float32(r["accuracy"]) == np.float32(hits.float().mean().item())


def test_wrapper_refuses_what_the_kernel_cannot_take():
    from tumblr_emotions_amd import ops
    from tumblr_emotions_amd.metrics import StreamingMetrics
    m = StreamingMetrics(15, "cuda")
    with pytest.raises(ValueError):
        m.update(torch.zeros(4, 14, device="cuda"), torch.zeros(4, dtype=torch.int64, device="cuda"))
    with pytest.raises(ValueError):
        m.update(torch.zeros(4, 15, device="cuda"), torch.zeros(4, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError):
        ops.eval_metrics_update(torch.zeros(4, 15, device="cuda"), torch.zeros(4, dtype=torch.int64, device="cuda"),
                                torch.zeros(10, dtype=torch.int64, device="cuda"), m.loss_sum, m._scratch)
    with pytest.raises(RuntimeError):
        StreamingMetrics(1025, "cuda")
    counts, loss = m.state()
    assert not counts.any() and loss[0] == 0.0
