"""Streaming evaluation metrics without a device: the two entry points are exported, bound and report argument errors before
any launch; metrics.summarize on a hand-written state; the config checker of the validation / metrics keys."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from tumblr_emotions_amd import _lib
    if not (os.path.exists(_lib.LIB_PATH) and os.path.exists(_lib.TUNING_LIB_PATH)):
        subprocess.run(["make", "-C", os.path.join(ROOT, "tumblr_emotions_amd", "csrc"), "-j4"], check=True)
    return _lib


def test_entry_points_are_exported_and_bound(lib):
    dll = ctypes.CDLL(lib.LIB_PATH)
    for name in ("ds_eval_metrics_workspace", "ds_eval_metrics_update"):
        assert hasattr(dll, name) and name in lib.SIGNATURES
        assert name in open(os.path.join(ROOT, "include", "ds_kernels.h")).read()
    from tumblr_emotions_amd import metrics, ops
    assert callable(ops.eval_metrics_update) and callable(metrics.StreamingMetrics)


def test_update_reports_argument_errors_before_any_launch(lib):
    l = lib.load()
    assert l.ds_eval_metrics_update(None, 15, None, 4, 15, None, None, None, None) == -1
    assert b"ds_eval_metrics_update" in l.ds_last_error()
    # non-null (host) pointers: the size checks come before anything is launched, so nothing dereferences them
    logits = (ctypes.c_float * 64)()
    labels = (ctypes.c_int64 * 4)()
    counts = (ctypes.c_int64 * (15 * 15 + 15 + 4))()
    loss = (ctypes.c_double * 1)()
    scratch = (ctypes.c_double * 8)()
    p = [ctypes.cast(a, ctypes.c_void_p) for a in (logits, labels, counts, loss, scratch)]
    for B, C, ldl in ((0, 15, 15), (65537, 15, 15), (4, 0, 15), (4, 1025, 1025), (4, 15, 14)):
        l.ds_gather_rows(None, None, None, 1, 1, 1, 1, 1, None)          # another entry point's name in the error text
        assert l.ds_eval_metrics_update(p[0], ldl, p[1], B, C, p[2], p[3], p[4], None) == -1, (B, C, ldl)
        assert b"ds_eval_metrics_update" in l.ds_last_error(), (B, C, ldl)
    for missing in range(5):
        q = list(p)
        q[missing] = None
        assert l.ds_eval_metrics_update(q[0], 15, q[1], 4, 15, q[2], q[3], q[4], None) == -1, missing


def test_workspace_answers_without_a_device(lib):
    l = lib.load()
    for B, C in ((1, 2), (257, 15), (4096, 15), (33, 1000), (65536, 1024), (65536, 1)):
        n = l.ds_eval_metrics_workspace(B, C)
        assert n >= 8 and n % 8 == 0, (B, C, n)
    assert l.ds_eval_metrics_workspace(4096, 15) >= l.ds_eval_metrics_workspace(257, 15)
    for B, C in ((0, 15), (65537, 15), (4, 0), (4, 1025), (-1, -1)):
        assert l.ds_eval_metrics_workspace(B, C) < 0, (B, C)


def test_summarize_hand_written_three_class_state():
    """Labels 0: 3 rows (2 predicted 0, 1 predicted 1); label 1: 2 rows (1 predicted 1, 1 predicted 0); class 2 has no
    support, and nothing is predicted as 2.  Ranks: the 3 correct rows rank 0, one wrong row rank 1, one rank 2."""
    from tumblr_emotions_amd.metrics import counts_size, summarize
    C = 3
    counts = np.zeros(counts_size(C), np.int64)
    counts[:9] = [2, 1, 0,
                  1, 1, 0,
                  0, 0, 0]
    counts[9:12] = [3, 1, 1]
    counts[12:15] = [5, 2, 1]            # n, n_nonfinite, n_bad_label
    r = summarize(counts, np.array([7.5]), C, top_k=(1, 2, 5))
    assert (r["n"], r["n_nonfinite"], r["n_bad_label"]) == (5, 2, 1)
    assert r["accuracy"] == 3 / 5
    assert r["top_k"] == {1: 3 / 5, 2: 4 / 5}            # k = 5 > C is left out
    assert r["loss"] == 1.5
    assert r["confusion"] == [[2, 1, 0], [1, 1, 0], [0, 0, 0]]
    pc = r["per_class"]
    assert pc["support"] == [3, 2, 0]
    assert pc["precision"] == pytest.approx([2 / 3, 1 / 2, 0.0], abs=1e-15)
    assert pc["recall"] == pytest.approx([2 / 3, 1 / 2, 0.0], abs=1e-15)
    assert pc["f1"] == pytest.approx([2 / 3, 1 / 2, 0.0], abs=1e-15)
    assert r["macro_f1"] == pytest.approx((2 / 3 + 1 / 2) / 2, abs=1e-15)      # class 2 (no support) is not averaged in
    import json
    back = json.loads(json.dumps(r))
    assert back["top_k"] == {"1": 3 / 5, "2": 4 / 5} and back["confusion"] == r["confusion"]
    # a class that is predicted but never the label: precision 0, recall with an empty denominator 0, outside macro-F1
    counts[:9] = [2, 0, 1,
                  0, 2, 0,
                  0, 0, 0]
    r = summarize(counts, np.array([0.0]), C)
    assert r["per_class"]["precision"] == pytest.approx([1.0, 1.0, 0.0]) and r["per_class"]["recall"] == pytest.approx([2 / 3, 1.0, 0.0])
    assert r["macro_f1"] == pytest.approx((0.8 + 1.0) / 2)
    # an empty state divides nothing by zero
    r = summarize(np.zeros(counts_size(C), np.int64), np.zeros(1), C)
    assert r["accuracy"] == 0.0 and r["loss"] == 0.0 and r["macro_f1"] == 0.0 and not math.isnan(r["top_k"][1])
    with pytest.raises(ValueError):
        summarize(np.zeros(5, np.int64), np.zeros(1), C)


def test_config_checker_refuses_each_bad_combination():
    from tumblr_emotions_amd.metrics import check_metrics_config
    good = [{}, {"validate_every": 1}, {"validate_every": 100, "validate_batches": 3, "keep_best": True, "metrics_top_k": (1, 2)},
            {"eval_metrics": True}, {"eval_metrics": True, "metrics_top_k": [1, 5]}, {"validate_every": 2, "keep_best": False},
            {"validate_every": 2, "eval_metrics": True, "validate_batches": 1}, {"eval_metrics": False}]
    for cfg in good:
        check_metrics_config(dict(cfg, batch_size=8))
    bad = [{"validate_every": 0}, {"validate_every": -3}, {"validate_every": True}, {"validate_every": 2.0}, {"validate_every": "5"},
           {"validate_every": 2, "validate_batches": 0}, {"validate_every": 2, "validate_batches": True},
           {"validate_every": 2, "validate_batches": 1.5},
           {"validate_batches": 3}, {"keep_best": True}, {"keep_best": False}, {"metrics_top_k": (1, 3)},
           {"eval_metrics": True, "validate_batches": 3}, {"eval_metrics": True, "keep_best": True},
           {"eval_metrics": False, "metrics_top_k": (1,)},
           {"validate_every": 2, "keep_best": 1}, {"validate_every": 2, "metrics_top_k": ()},
           {"validate_every": 2, "metrics_top_k": (0, 1)}, {"validate_every": 2, "metrics_top_k": 3},
           {"validate_every": 2, "metrics_top_k": (True,)}]
    for cfg in bad:
        with pytest.raises(ValueError):
            check_metrics_config(cfg)


def test_front_ends_check_the_keys_at_construction_without_a_device():
    """The models call the checker before anything touches the device: a bad key is a ValueError here too."""
    from tumblr_emotions_amd.text_model.text_embedding import _CONFIG, TextModel
    cfg = dict(_CONFIG, batch_size=8, rnn_size=32, vocab_size=60, embedding_dim=20, post_size=12, num_samples=24, synthetic=True)
    for extra in ({"validate_every": 0}, {"validate_batches": 2}, {"keep_best": True}, {"metrics_top_k": (1,)}):
        with pytest.raises(ValueError, match="validate_every|validate_batches|keep_best|metrics_top_k"):
            TextModel(dict(cfg, **extra))
