"""Validation during training (config['validate_every']) and streaming metrics in evaluate_* (config['eval_metrics']) through
the three front ends: what is written and when, that a validation line equals what evaluate_* reports for the checkpoint of
that step, and that validation changes nothing about training -- variables, Adam slots and moving statistics bit for bit."""
import json
import os
import socket

import numpy as np
import pytest
import torch

from test_frontends_gpu import SMALL_TEXT

pytestmark = pytest.mark.gpu

STEPS, M = 7, 3
VALID = dict(SMALL_TEXT, validate_every=3, validate_batches=M, keep_best=True)
JOINT = dict(SMALL_TEXT, batch_size=4, num_samples=8)


def _lines(path):
    with open(path) as f:
        return [json.loads(l) for l in f if l.strip()]


def _final(train_dir, steps):
    """Everything save_checkpoint wrote after the last step: variables (moving statistics among them) and the Adam slots."""
    ck = torch.load(os.path.join(train_dir, "model.ckpt-%d.pt" % steps), map_location="cpu", weights_only=True)
    assert ck["global_step"] == steps
    out = {k: v.numpy() for k, v in ck["variables"].items()}
    out["adam_m"], out["adam_v"] = ck["adam_m"].numpy(), ck["adam_v"].numpy()
    return out


def _assert_same_bits(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, k
        assert a[k].tobytes() == b[k].tobytes(), k


@pytest.fixture(scope="module")
def text_runs(tmp_path_factory):
    """Two plain 7-step runs of the text model (the control) and one with validate_every=3, keep_best."""
    from tumblr_emotions_amd.text_model.text_embedding import train_text_model
    root = tmp_path_factory.mktemp("validation")
    dirs = {name: str(root / name) for name in ("plain_a", "plain_b", "valid")}
    train_text_model(dirs["plain_a"], STEPS, config=SMALL_TEXT, quiet=True)
    train_text_model(dirs["plain_b"], STEPS, config=SMALL_TEXT, quiet=True)
    train_text_model(dirs["valid"], STEPS, config=VALID, quiet=True)
    return dirs


def test_without_the_keys_nothing_new_is_written(text_runs, tmp_path):
    from tumblr_emotions_amd.text_model.text_embedding import evaluate_text_model
    for name in ("validation.jsonl", "model.best.pt", "best.json"):
        assert not os.path.exists(os.path.join(text_runs["plain_a"], name)), name
    evaluate_text_model(text_runs["plain_a"], str(tmp_path), "validation", 2, config=SMALL_TEXT, quiet=True)
    assert os.path.exists(tmp_path / "validation" / "accuracy.jsonl")
    assert not os.path.exists(tmp_path / "validation" / "metrics.jsonl")


def test_validation_lines_at_every_third_step_and_the_last(text_runs):
    lines = _lines(os.path.join(text_runs["valid"], "validation.jsonl"))
    assert [l["global_step"] for l in lines] == [3, 6, 7]
    for l in lines:
        assert l["n"] == M * SMALL_TEXT["batch_size"] and l["n_nonfinite"] == 0 and l["n_bad_label"] == 0
        assert sum(map(sum, l["confusion"])) == l["n"] and sum(l["per_class"]["support"]) == l["n"]
        assert sorted(l["top_k"]) == ["1", "3", "5"] and l["top_k"]["1"] == l["accuracy"]
        assert np.isfinite(l["loss"]) and l["loss"] > 0
    assert lines[0]["learning_rate"] == 1e-3 and lines[1]["learning_rate"] == pytest.approx(3e-4)     # 24 / 8: an epoch is 3 steps
    assert lines[0]["per_class"]["support"] == lines[2]["per_class"]["support"]        # the same batches every time


def test_last_line_equals_evaluation_of_the_final_checkpoint(text_runs, tmp_path, capsys):
    from tumblr_emotions_amd.text_model.text_embedding import evaluate_text_model
    last = _lines(os.path.join(text_runs["valid"], "validation.jsonl"))[-1]
    acc = evaluate_text_model(text_runs["valid"], str(tmp_path), "validation", M, config=dict(VALID, eval_metrics=True), quiet=True)
    assert "WARNING" not in capsys.readouterr().out
    (line,) = _lines(tmp_path / "validation" / "metrics.jsonl")
    assert (line["global_step"], line["num_evals"], line["mode"]) == (STEPS, M, "validation")
    for key in ("n", "n_nonfinite", "n_bad_label", "confusion"):
        assert line[key] == last[key], key
    assert line["per_class"]["support"] == last["per_class"]["support"]
    assert line["loss"] == last["loss"] and line["accuracy"] == last["accuracy"] == acc
    # the return value and accuracy.jsonl are what they are without the key
    plain = evaluate_text_model(text_runs["valid"], str(tmp_path / "plain"), "validation", M, config=VALID, quiet=True)
    assert isinstance(acc, float) and acc == plain
    with_key, without = _lines(tmp_path / "validation" / "accuracy.jsonl"), _lines(tmp_path / "plain" / "validation" / "accuracy.jsonl")
    assert with_key == without
    assert not os.path.exists(tmp_path / "plain" / "validation" / "metrics.jsonl")
    # mode 'train' (batch statistics and dropout stay on) takes the key as well
    acc_t = evaluate_text_model(text_runs["valid"], str(tmp_path), "train", 2, config=dict(SMALL_TEXT, eval_metrics=True), quiet=True)
    (line_t,) = _lines(tmp_path / "train" / "metrics.jsonl")
    assert line_t["mode"] == "train" and line_t["n"] == 2 * SMALL_TEXT["batch_size"] and line_t["accuracy"] == acc_t


def test_validation_leaves_text_training_bit_identical(text_runs, tmp_path):
    from tumblr_emotions_amd.text_model.text_embedding import train_text_model
    control = _final(text_runs["plain_a"], STEPS)
    _assert_same_bits(control, _final(text_runs["plain_b"], STEPS))               # the control: two plain runs agree
    _assert_same_bits(control, _final(text_runs["valid"], STEPS))
    d = str(tmp_path / "every2")
    train_text_model(d, STEPS, config=dict(SMALL_TEXT, validate_every=2), quiet=True)
    assert [l["global_step"] for l in _lines(os.path.join(d, "validation.jsonl"))] == [2, 4, 6, 7]
    assert _lines(os.path.join(d, "validation.jsonl"))[0]["n"] == 10 * SMALL_TEXT["batch_size"]      # validate_batches defaults to 10
    _assert_same_bits(control, _final(d, STEPS))


@pytest.mark.parametrize("extra", [{}, {"frozen_bn": True, "fused_inference": True}], ids=["batch_stats", "frozen_bn_fused"])
def test_validation_leaves_joint_training_bit_identical(tmp_path, extra):
    """fp32 joint model, validate_every=1: the moving statistics are variables of the checkpoint and are compared too."""
    from tumblr_emotions_amd.image_text_model.im_text_rnn_model import train_deep_sentiment
    cfg = dict(JOINT, **extra)
    dirs = [str(tmp_path / n) for n in ("a", "b", "v")]
    train_deep_sentiment(None, dirs[0], 3, config=cfg, quiet=True)
    train_deep_sentiment(None, dirs[1], 3, config=cfg, quiet=True)
    train_deep_sentiment(None, dirs[2], 3, config=dict(cfg, validate_every=1, validate_batches=2), quiet=True)
    control = _final(dirs[0], 3)
    assert any(k.endswith("moving_mean") for k in control) and any(k.endswith("moving_variance") for k in control)
    _assert_same_bits(control, _final(dirs[1], 3))
    _assert_same_bits(control, _final(dirs[2], 3))
    lines = _lines(os.path.join(dirs[2], "validation.jsonl"))
    assert [l["global_step"] for l in lines] == [1, 2, 3] and all(l["n"] == 8 for l in lines)
    # the last line is what evaluate_deep_sentiment reports for the final checkpoint (with fused_inference where configured)
    from tumblr_emotions_amd.image_text_model.im_text_rnn_model import evaluate_deep_sentiment
    acc = evaluate_deep_sentiment(dirs[2], str(tmp_path / "log"), "validation", 2, config=dict(cfg, eval_metrics=True), quiet=True)
    (line,) = _lines(tmp_path / "log" / "validation" / "metrics.jsonl")
    assert line["confusion"] == lines[-1]["confusion"] and line["loss"] == lines[-1]["loss"] and acc == lines[-1]["accuracy"]


def test_image_model_takes_both_keys(tmp_path):
    from tumblr_emotions_amd.image_model.im_model import evaluate_image_model, train_image_model
    cfg = dict(batch_size=4, num_samples=8, synthetic=True)
    d = str(tmp_path / "image")
    train_image_model(None, d, 2, config=dict(cfg, validate_every=1, validate_batches=1), quiet=True)
    lines = _lines(os.path.join(d, "validation.jsonl"))
    assert [l["global_step"] for l in lines] == [1, 2] and all(l["n"] == 4 for l in lines)
    acc = evaluate_image_model(d, str(tmp_path / "log"), "validation", 1, config=dict(cfg, eval_metrics=True), quiet=True)
    (line,) = _lines(tmp_path / "log" / "validation" / "metrics.jsonl")
    assert line["confusion"] == lines[-1]["confusion"] and line["loss"] == lines[-1]["loss"] and acc == lines[-1]["accuracy"]


def test_keep_best_writes_a_loadable_checkpoint_beside_the_index(text_runs):
    from tumblr_emotions_amd.text_model.text_embedding import _CONFIG, TextModel
    from tumblr_emotions_amd.training import latest_checkpoint, load_checkpoint
    d = text_runs["valid"]
    lines = _lines(os.path.join(d, "validation.jsonl"))
    accs = [l["accuracy"] for l in lines]
    first_max = lines[int(np.argmax(accs))]                    # argmax takes the first maximum: only a strict gain replaces
    with open(os.path.join(d, "best.json")) as f:
        best = json.load(f)
    assert best == {"global_step": first_max["global_step"], "accuracy": first_max["accuracy"]}
    model = TextModel(dict(_CONFIG, **VALID))
    assert load_checkpoint(model, os.path.join(d, "model.best.pt")) == best["global_step"]
    ck = torch.load(os.path.join(d, "model.best.pt"), map_location="cpu", weights_only=True)
    assert sorted(ck) == sorted(torch.load(os.path.join(d, "model.ckpt-%d.pt" % STEPS), map_location="cpu", weights_only=True))
    with open(os.path.join(d, "checkpoint")) as f:
        assert json.load(f) == {"model_checkpoint_path": "model.ckpt-%d.pt" % STEPS, "global_step": STEPS}
    assert latest_checkpoint(d) == os.path.join(d, "model.ckpt-%d.pt" % STEPS)


def _real_dataset(root):
    from test_datasets_cpu import _make_dataset
    os.makedirs(root)
    _make_dataset(root, n_train=9, n_valid=4)
    rng = np.random.RandomState(3)
    glove = rng.normal(0, 0.4, size=(100, 20)).astype(np.float32)
    os.makedirs(os.path.join(root, "text_model", "embedding_weights"))
    with open(os.path.join(root, "text_model", "embedding_weights", "glove.test.20d.txt"), "w") as f:
        for i, row in enumerate(glove):
            f.write("w%d %s\n" % (i, " ".join(repr(float(v)) for v in row)))
    return dict(dataset_dir=root, text_dir=os.path.join(root, "text_model"), emb_dir="embedding_weights",
                filename="glove.test.20d.txt", batch_size=4, rnn_size=32, post_size=50)


@pytest.fixture(scope="module")
def real_runs(tmp_path_factory):
    """Joint model on a converted dataset (9 train, 4 validation records, batch 4), 2 steps: without the key, and with
    validate_every=1 once per input pipeline."""
    from tumblr_emotions_amd.image_text_model.im_text_rnn_model import train_deep_sentiment
    root = tmp_path_factory.mktemp("real")
    cfg = _real_dataset(str(root / "data"))
    dirs = {name: str(root / name) for name in ("plain", "host", "device")}
    train_deep_sentiment(None, dirs["plain"], 2, config=cfg, quiet=True)
    for pipeline in ("host", "device"):
        train_deep_sentiment(None, dirs[pipeline], 2, quiet=True,
                             config=dict(cfg, validate_every=1, input_pipeline=pipeline, input_workers=4))
    return dirs


@pytest.mark.parametrize("pipeline", ["host", "device"])
def test_real_dataset_validation_reads_the_validation_split_and_not_the_training_stream(real_runs, pipeline):
    lines = _lines(os.path.join(real_runs[pipeline], "validation.jsonl"))
    assert [l["global_step"] for l in lines] == [1, 2]
    # one pass over the 4 validation records = one batch of 4, labels i % 3: the same batch at both validations
    assert all(l["n"] == 4 and l["per_class"]["support"] == [2, 1, 1] for l in lines)
    # both pipelines read identical batches: the same lines
    assert lines == _lines(os.path.join(real_runs["host"], "validation.jsonl"))
    # the training loader's stream was not consumed: the final variables are those of the run without the key
    _assert_same_bits(_final(real_runs["plain"], 2), _final(real_runs[pipeline], 2))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _dp_worker(rank, world, port, root, out):
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    import torch.distributed as dist
    from tumblr_emotions_amd import dp
    dp.init_distributed("gloo", device=0, rank=rank, world_size=world)
    try:
        from tumblr_emotions_amd.text_model.text_embedding import train_text_model
        cfg = dict(SMALL_TEXT, batch_size=4)
        train_text_model(os.path.join(root, "plain"), 4, config=cfg, quiet=True)
        dist.barrier()                     # rank 0 wipes and re-creates the next train_dir: nobody is still in the old one
        train_text_model(os.path.join(root, "valid"), 4, config=dict(cfg, validate_every=2, validate_batches=2), quiet=True)
        dist.barrier()
        out.put(rank)
    finally:
        dist.destroy_process_group()


def test_two_rank_training_validates_on_rank_0_only(tmp_path):
    import torch.multiprocessing as mp
    from test_dp_gpu import _collect
    ctx = mp.get_context("spawn")
    out = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, str(tmp_path), out)) for r in range(2)]
    for p in procs:
        p.start()
    assert sorted(_collect(out, procs, 2)) == [0, 1]                    # both ranks finish
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    lines = _lines(tmp_path / "valid" / "validation.jsonl")
    assert [l["global_step"] for l in lines] == [2, 4]                  # one writer: a second rank would double the lines
    assert all(l["n"] == 2 * 4 for l in lines)                          # global-order batches of batch_size, rank 0 / world 1
    _assert_same_bits(_final(str(tmp_path / "plain"), 4), _final(str(tmp_path / "valid"), 4))
