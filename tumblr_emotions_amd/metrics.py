"""Streaming evaluation metrics: confusion matrix, per-class precision / recall / F1, top-k accuracy and the held-out
cross-entropy, accumulated on the device by ds_eval_metrics_update (csrc/metrics.hip) and summarised on the host.

The reference reports one number, slim's streaming_accuracy (im_text_rnn_model.py:171-207); its 15 emotions are very unequal
classes, so the questions a maintainer asks first -- which emotions are taken for which -- need the whole matrix.
StreamingMetrics keeps the accumulators in device memory: update() enqueues one call and reads nothing back, state() is the
only copy.  summarize() and check_metrics_config() are pure functions of host data and need no device."""
import numpy as np

DEFAULT_TOP_K = (1, 3, 5)
_MAX_ROWS = 65536                  # ds_eval_metrics_update's largest batch


def counts_size(num_classes):
    """int64 words of the integer accumulator: confusion[C*C], rank_hist[C], n, n_nonfinite, n_bad_label, one reserved 0."""
    return num_classes * num_classes + num_classes + 4


def _is_count(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_)) and v > 0


def check_top_k(top_k):
    try:
        ks = tuple(top_k)
    except TypeError:
        ks = None
    if not ks or not all(_is_count(k) for k in ks):
        raise ValueError("metrics_top_k must be a non-empty sequence of positive ints, not %r" % (top_k,))
    return tuple(int(k) for k in ks)


def check_metrics_config(config):
    """The validation / metrics keys of a front-end config: config['eval_metrics'] (evaluate_*: streaming metrics and
    <log_dir>/<mode>/metrics.jsonl), config['validate_every'] = N (train_*: validate after every N-th step and after the last),
    config['validate_batches'] = M (default 10), config['keep_best'] (default False: model.best.pt + best.json) and
    config['metrics_top_k'] (default (1, 3, 5)).  A ValueError for a value that is not what the key takes, and for a key
    that would silently do nothing: validate_batches / keep_best without validate_every, metrics_top_k without validate_every
    or eval_metrics."""
    every = config.get("validate_every")
    if every is not None and not _is_count(every):
        raise ValueError("config['validate_every'] must be a positive int, not %r" % (every,))
    if "validate_batches" in config and not _is_count(config["validate_batches"]):
        raise ValueError("config['validate_batches'] must be a positive int, not %r" % (config["validate_batches"],))
    if "keep_best" in config and not isinstance(config["keep_best"], (bool, np.bool_)):
        raise ValueError("config['keep_best'] must be True or False, not %r" % (config["keep_best"],))
    if "metrics_top_k" in config:
        check_top_k(config["metrics_top_k"])
    for key in ("validate_batches", "keep_best"):
        if key in config and every is None:
            raise ValueError("config[%r] needs config['validate_every']: without it no validation runs" % key)
    if "metrics_top_k" in config and every is None and not config.get("eval_metrics", False):
        raise ValueError("config['metrics_top_k'] needs config['validate_every'] or config['eval_metrics']")


def _ratio(num, den):
    num, den = np.asarray(num, np.float64), np.asarray(den, np.float64)
    return np.divide(num, den, out=np.zeros_like(num), where=den > 0)


def summarize(counts, loss_sum, num_classes, top_k=DEFAULT_TOP_K):
    """The accumulators of ds_eval_metrics_update as a plain dict (NumPy on the host; JSON-serialisable): n, n_nonfinite,
    n_bad_label, accuracy, top_k {k: value} for each k <= num_classes, loss (mean cross-entropy over n), confusion (list of
    lists, row = label, column = prediction), per_class {support, precision, recall, f1} (an empty denominator gives 0.0)
    and macro_f1 over the classes with support > 0."""
    C = int(num_classes)
    counts = np.asarray(counts).reshape(-1)
    if counts.size != counts_size(C):
        raise ValueError("summarize: %d counts, expected %d for %d classes" % (counts.size, counts_size(C), C))
    counts = counts.astype(np.int64)
    conf = counts[:C * C].reshape(C, C)
    rank_hist = counts[C * C:C * C + C]
    n, n_nonfinite, n_bad = (int(v) for v in counts[C * C + C:C * C + C + 3])
    tp = np.diag(conf)
    support, predicted = conf.sum(axis=1), conf.sum(axis=0)
    precision, recall = _ratio(tp, predicted), _ratio(tp, support)
    f1 = _ratio(2.0 * precision * recall, precision + recall)
    present = support > 0
    return {
        "n": n, "n_nonfinite": n_nonfinite, "n_bad_label": n_bad,
        "accuracy": int(rank_hist[0]) / n if n else 0.0,
        "top_k": {int(k): (int(rank_hist[:k].sum()) / n if n else 0.0) for k in check_top_k(top_k) if k <= C},
        "loss": float(np.asarray(loss_sum, np.float64).reshape(-1)[0]) / n if n else 0.0,
        "confusion": conf.tolist(),
        "per_class": {"support": support.tolist(), "precision": precision.tolist(), "recall": recall.tolist(),
                      "f1": f1.tolist()},
        "macro_f1": float(f1[present].mean()) if present.any() else 0.0,
    }


class StreamingMetrics:
    """Accumulators of ds_eval_metrics_update for `num_classes` classes on `device`, and the kernel's scratch.  update() adds a
    batch on the current stream and reads nothing back; reset() zeroes on the device; state() is one copy to the host and the
    only synchronisation; result() is summarize(state())."""

    def __init__(self, num_classes, device="cuda", top_k=DEFAULT_TOP_K):
        import torch
        from . import ops
        self.num_classes = int(num_classes)
        self.top_k = check_top_k(top_k)
        scratch_bytes = ops.eval_metrics_workspace(_MAX_ROWS, self.num_classes)      # raises for num_classes outside [1, 1024]
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("tumblr_emotions_amd kernels need CUDA/HIP tensors; there is no CPU fallback")
        n = counts_size(self.num_classes)
        self._buf = torch.zeros(n + 1, dtype=torch.int64, device=device)      # counts, then the loss sum's 8 bytes: one copy
        self.counts = self._buf[:n]
        self.loss_sum = self._buf[n:].view(torch.float64)
        self._scratch = torch.empty(scratch_bytes // 8, dtype=torch.float64, device=device)

    def update(self, logits, labels):
        import torch
        from . import ops
        if logits.dtype != torch.float32:
            logits = logits.float()
        if logits.dim() == 2 and logits.stride(1) != 1:
            logits = logits.contiguous()
        if logits.dim() != 2 or logits.shape[1] != self.num_classes:
            raise ValueError("StreamingMetrics.update: logits must be [B, %d], not %s" % (self.num_classes, tuple(logits.shape)))
        ops.eval_metrics_update(logits, labels.contiguous(), self.counts, self.loss_sum, self._scratch)

    def reset(self):
        self._buf.zero_()

    def state(self):
        host = self._buf.cpu().numpy()
        return host[:-1], host[-1:].view(np.float64)

    def result(self):
        counts, loss_sum = self.state()
        return summarize(counts, loss_sum, self.num_classes, self.top_k)
