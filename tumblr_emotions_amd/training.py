"""The training loop the reference delegates to `slim.learning.train`, shared by
train_image_model / train_text_model / train_deep_sentiment.

Behaviour kept from the reference (image_text_model/im_text_rnn_model.py:107-169):
  * `train_dir` is deleted and re-created (no resume)                                   :116-119
  * learning rate = initial_lr * decay_factor**epoch, re-assigned whenever
    step % (num_samples / batch_size) == 0                                             :137-147
  * a checkpoint every `save_interval_secs` (600 s) and at the end                      :160-167
  * log line `global step N: loss = L (S sec/step)` (slim train_step)                   A11
  * prints `Finished training. Last batch loss {:.3f}`                                  :169
The per-step work itself is SentimentNet.train_step (HIP kernels).
"""
import contextlib
import json
import os
import shutil
import time

import numpy as np
import torch

from .feature_cache import check_feature_cache_config
from .metrics import check_metrics_config
from .synthetic import synthetic_batch_numpy, to_device


def check_clones_config(config):
    """config['num_clones'] = K (default 1; train_*): every rank trains K of slim's in-graph clones per step, one after the
    other, with their gradients accumulated (SentimentNet.train_step(num_clones=K)).  config['batch_size']
    stays the batch of ONE clone, so a rank reads batch_size * K samples per step.  Returns K.  Needs no device.  ValueError
    for anything but a positive int (a bool is not one); with K > 1, config['sync_bn'] is a ValueError (clones have their own
    BatchNorm statistics by definition) and a config['dtype'] other than 'f32' a NotImplementedError."""
    K = config.get("num_clones", 1)
    if isinstance(K, (bool, np.bool_)) or not isinstance(K, (int, np.integer)) or K < 1:
        raise ValueError("config['num_clones'] must be a positive int, not %r" % (K,))
    K = int(K)
    if K > 1:
        if config.get("sync_bn", False):
            raise ValueError("config['num_clones'] = %d with config['sync_bn']: clones have their own BatchNorm statistics "
                             "by definition" % K)
        if config.get("dtype", "f32") != "f32":
            raise NotImplementedError("config['num_clones'] = %d with config['dtype'] = %r: clones are implemented for the "
                                      "fp32 configuration" % (K, config["dtype"]))
    return K


def clip_net_kwargs(config):
    """The gradient-clipping keys of a front-end config as SentimentNet arguments; needs no device.
    config['clip_gradient_norm'] = c: slim's create_train_op(clip_gradient_norm=c), tf.clip_by_norm per variable;
    config['clip_global_norm'] = c: tf.clip_by_global_norm; config['skip_nonfinite_steps'] = True: a step whose gradient
    has a NaN / Inf norm leaves the variables and the Adam slots alone.  config['log_gradient_norms'] = True: run_training
    appends net.grad_norms() to <train_dir>/gradients.jsonl on its logging steps -- a ValueError without one of the other
    three keys, which are what makes the step compute norms (skip_nonfinite_steps is the one that changes no finite step).
    ValueError for both thresholds at once, a threshold that is not a finite number > 0, or a flag that is not a bool."""
    from .net import check_clip_config
    kw = {k: config[k] for k in ("clip_gradient_norm", "clip_global_norm") if config.get(k) is not None}
    check_clip_config(**kw)
    for k in ("skip_nonfinite_steps", "log_gradient_norms"):
        if not isinstance(config.get(k, False), (bool, np.bool_)):
            raise ValueError("config[%r] must be a bool, not %r" % (k, config[k]))
    if config.get("skip_nonfinite_steps", False):
        kw["skip_nonfinite_steps"] = True
    if config.get("log_gradient_norms", False) and not kw:
        raise ValueError("config['log_gradient_norms'] needs config['clip_gradient_norm'], config['clip_global_norm'] or "
                         "config['skip_nonfinite_steps']: without them the step computes no gradient norm")
    return kw


def ema_net_kwargs(config):
    """config['moving_average_decay'] = d as a SentimentNet argument; needs no device.  slim's
    --moving_average_decay: train_* keep moving averages of the trained variables (decay min(d, (1 + t) / (10 + t))) and
    write them into every checkpoint; evaluate_*, the analyses and class_visualisation given the key restore the averages
    in place of the variables, as slim's eval does when its flag is set.  ValueError unless d is a float with 0 < d < 1;
    with a config['dtype'] other than 'f32' a NotImplementedError."""
    from .net import check_ema_config
    d = check_ema_config(config.get("moving_average_decay"))
    if d is None:
        return {}
    if config.get("dtype", "f32") != "f32":
        raise NotImplementedError("config['moving_average_decay'] with config['dtype'] = %r: moving averages are implemented "
                                  "for the fp32 configuration" % (config["dtype"],))
    return {"moving_average_decay": d}


def loss_net_kwargs(config):
    """config['label_smoothing'] and config['class_weights'] as SentimentNet arguments; needs no device.
    slim's --label_smoothing and the `weights` of slim.losses.softmax_cross_entropy: label_smoothing = e trains on
    onehot (1 - e) + e / C; class_weights = [w_0 .. w_{C-1}] weighs a row's loss by its label's weight and divides by the
    number of rows whose weight is not zero.  What net.check_loss_config refuses is refused here (the number of weights is
    held against the data set's classes when the net is built).  label_smoothing = 0 (or absent) without weights returns {}:
    the step is the one without the keys.  train_* pass them to the net; evaluate_*, the analyses, explain_posts and
    class_visualisation ignore them, and validation during training keeps the plain mean cross entropy."""
    from .net import check_loss_config
    eps, cw = check_loss_config(config.get("label_smoothing"), config.get("class_weights"), nb_emotions=None)
    kw = {}
    if eps != 0.0:
        kw["label_smoothing"] = eps
    if cw is not None:
        kw["class_weights"] = list(cw)
    return kw


_OPT_KEYS = ("opt_epsilon", "momentum", "rmsprop_decay", "adam_beta1", "adam_beta2")


def optimizer_net_kwargs(config):
    """The optimiser keys of a front-end config as SentimentNet arguments; needs no device.  slim's
    --optimizer block: config['optimizer'] in 'adam' (default, the reference's), 'sgd', 'momentum', 'rmsprop';
    config['opt_epsilon'], config['momentum'], config['rmsprop_decay'], config['adam_beta1'], config['adam_beta2'].  What
    net.check_optimizer_config refuses is refused here, and so is ANY of the five keys present for an optimiser that does not
    read it, default value or not.  train_* pass them to the net; evaluate_*, the analyses and class_visualisation build
    their net without them (they run no optimiser and load any checkpoint)."""
    from .net import _OPT_HYPER, check_optimizer_config
    name = config.get("optimizer", "adam")
    kw = {k: config[k] for k in _OPT_KEYS if k in config}
    check_optimizer_config(name, **kw)
    for k in kw:
        if name not in _OPT_HYPER[k][1]:
            raise ValueError("config[%r] is given, but config['optimizer'] = %r does not read it" % (k, name))
    if "optimizer" in config:
        kw["optimizer"] = name
    return kw


_SCHEDULE_KEYS = {"learning_rate_decay_factor": ("exponential",), "num_epochs_per_decay": ("exponential", "polynomial"),
                  "end_learning_rate": ("polynomial",)}
_SCHEDULE_DEFAULTS = {"learning_rate_decay_factor": 0.94, "num_epochs_per_decay": 2.0, "end_learning_rate": 1e-4}


def check_schedule_config(config, num_samples=None):
    """config['learning_rate_decay_type'] and its keys (slim's train_image_classifier.py:221-258); needs no device.  Returns
    None when the type is absent -- the reference's per-epoch rule stays -- else (type, decay_steps or None).
      'fixed'        initial_lr
      'exponential'  initial_lr * learning_rate_decay_factor (0.94) ** floor(t / decay_steps), slim's staircase
      'polynomial'   (initial_lr - end_learning_rate (1e-4)) * (1 - min(t, decay_steps) / decay_steps) + end_learning_rate
    decay_steps = int(num_samples / batch_size * num_epochs_per_decay (2.0)), slim's formula taken literally: batch_size is ONE
    clone's, so with num_clones or several ranks an "epoch" of the schedule is num_clones * world passes over the data (slim
    has the same quirk).  ValueError for an unknown type, a schedule key without the type or for a type that does not read
    it, a value out of range (factor > 0, epochs > 0, end >= 0; finite numbers, a bool is not one) and decay_steps == 0
    (checked when num_samples is given)."""
    kind = config.get("learning_rate_decay_type")
    given = [k for k in _SCHEDULE_KEYS if k in config]
    if kind is None:
        if given:
            raise ValueError("config[%r] needs config['learning_rate_decay_type']: without it the learning rate follows "
                             "initial_lr * decay_factor ** epoch" % given[0])
        return None
    if kind not in ("fixed", "exponential", "polynomial"):
        raise ValueError("config['learning_rate_decay_type'] must be 'fixed', 'exponential' or 'polynomial', not %r" % (kind,))
    for k in given:
        x = config[k]
        if kind not in _SCHEDULE_KEYS[k]:
            raise ValueError("config[%r] is given, but config['learning_rate_decay_type'] = %r does not read it" % (k, kind))
        if isinstance(x, (bool, np.bool_)) or not isinstance(x, (int, float, np.integer, np.floating)) or not np.isfinite(x) \
                or (x < 0 if k == "end_learning_rate" else not x > 0):
            raise ValueError("config[%r] must be a finite number %s, not %r" % (k, ">= 0" if k == "end_learning_rate" else "> 0", x))
    if kind == "fixed" or num_samples is None:
        return kind, None
    decay_steps = int(num_samples / config["batch_size"] * config.get("num_epochs_per_decay", 2.0))
    if decay_steps == 0:
        raise ValueError("config['learning_rate_decay_type'] = %r: decay_steps = int(num_samples / batch_size * "
                         "num_epochs_per_decay) = int(%d / %d * %r) is 0" % (kind, num_samples, config["batch_size"],
                                                                              config.get("num_epochs_per_decay", 2.0)))
    return kind, decay_steps


def learning_rate_at(config, num_samples, t, world=1):
    """The learning rate of the step that follows t completed steps (TF reads global_step before the increment, so a resumed
    run continues the schedule from the checkpoint's step).  A pure function of its arguments; needs no device.
    Without config['learning_rate_decay_type']: the reference's rule as run_training has always applied it, a Python float --
    initial_lr * decay_factor ** (t // nb_batches), nb_batches = max(1, num_samples // (batch_size * num_clones * world)).
    With it (check_schedule_config): an np.float32 formed the way tf.train.exponential_decay / polynomial_decay form theirs --
    every hyper-parameter and the step cast to fp32, every operation rounded to fp32 once, in TF's order:
      exponential  p = floor(t / decay_steps); initial_lr * pow(factor, p)          (the power: correctly rounded)
      polynomial   p = min(t, decay_steps) / decay_steps; (initial_lr - end) * (1 - p) + end"""
    sched = check_schedule_config(config, num_samples)
    if sched is None:
        nb_batches = max(1, num_samples // (config["batch_size"] * check_clones_config(config) * world))
        return config["initial_lr"] * config["decay_factor"] ** (t // nb_batches)
    f32 = np.float32
    kind, decay_steps = sched
    lr0 = f32(config["initial_lr"])
    if kind == "fixed":
        return lr0
    gs, ds = f32(t), f32(decay_steps)
    if kind == "exponential":
        p = np.floor(f32(gs / ds))
        return f32(lr0 * f32(float(f32(config.get("learning_rate_decay_factor", 0.94))) ** float(p)))
    end = f32(config.get("end_learning_rate", 1e-4))
    p = f32(min(gs, ds) / ds)
    return f32(f32(f32(lr0 - end) * f32(f32(1.0) - p)) + end)


def _log_gradient_norms(net, train_dir, step):
    """One line of <train_dir>/gradients.jsonl: the step, the global norm, the factor(s), the skipped count, the norms."""
    gn = net.grad_norms()
    line = {"global_step": step, "global_norm": gn.pop("global_norm"), "nonfinite": gn.pop("nonfinite"),
            "skipped_steps": gn.pop("skipped_steps")}
    for k in ("factor", "factors"):
        if k in gn:
            line[k] = gn.pop(k)
    line["norms"] = gn
    with open(os.path.join(train_dir, "gradients.jsonl"), "a") as f:
        f.write(json.dumps(line) + "\n")


def _rank_world():
    if torch.distributed.is_available() and torch.distributed.is_initialized():
        return torch.distributed.get_rank(), torch.distributed.get_world_size()
    return 0, 1


def _write_checkpoint(model, path, step):
    net = model.net
    torch.cuda.synchronize()
    # plain tensors / numbers / strings only, so that the file loads with weights_only=True
    ck = {"variables": {k: torch.from_numpy(v) for k, v in net.state_dict().items()},
          "adam_m": net.store.m.cpu(), "adam_v": net.store.v.cpu(), "global_step": int(step),
          "config": json.dumps(model.config, default=str)}
    if not net._reference_adam:      # the optimiser's name and hyper-parameters; a file without the key is the reference's adam
        ck["optimizer"] = dict(net.opt)      # (the slots stay under adam_m / adam_v: slot0 / slot1 of every kind)
    if net.ce_desc is not None:      # label_smoothing / class_weights, for the record: the loss has no state to restore
        ck["loss"] = {"label_smoothing": float(net.label_smoothing),
                      "class_weights": None if net.class_weights is None else [float(w) for w in net.class_weights]}
    if net.store.ema is not None:      # moving_average_decay: the averages of the trainable variables, under their TF names
        ck["moving_averages"] = {k: torch.from_numpy(v) for k, v in net.averages_state_dict().items()}
    torch.save(ck, path)


def save_checkpoint(model, train_dir, step):
    """Variables under their TF names + Adam slots + step, as one torch file per checkpoint."""
    path = os.path.join(train_dir, "model.ckpt-%d.pt" % step)
    _write_checkpoint(model, path, step)
    with open(os.path.join(train_dir, "checkpoint"), "w") as f:
        json.dump({"model_checkpoint_path": os.path.basename(path), "global_step": step}, f)
    return path


def latest_checkpoint(checkpoint_dir):
    idx = os.path.join(checkpoint_dir, "checkpoint")
    if not os.path.exists(idx):
        return None
    with open(idx) as f:
        return os.path.join(checkpoint_dir, json.load(f)["model_checkpoint_path"])


class Validator:
    """config['validate_every'] = N: held-out metrics during training (rank 0 only; no collective is involved).  run() feeds
    model.validation_batches(config['validate_batches']) -- the same batches every time -- through net.predict(is_training=
    False), which writes no variable, moving statistic, pivot or step counter, into a freshly reset StreamingMetrics, and
    appends result() + global_step + learning_rate to <train_dir>/validation.jsonl.  config['keep_best']: an accuracy strictly
    above the best so far also writes model.best.pt (what save_checkpoint writes; the `checkpoint` index is left alone, so
    latest_checkpoint does not see it) and best.json.
    A net with moving averages (config['moving_average_decay']) is validated inside net.averaged_weights(): on the averages,
    what evaluate_* will score; every line then carries "weights": "averaged".  model.best.pt is written
    outside the context and holds variables and averages like any other checkpoint."""

    def __init__(self, model, train_dir):
        from .metrics import DEFAULT_TOP_K, StreamingMetrics
        cfg = model.config
        self.model, self.train_dir = model, train_dir
        self.every = int(cfg["validate_every"])
        self.batches = int(cfg.get("validate_batches", 10))
        self.keep_best = bool(cfg.get("keep_best", False))
        self.fused = bool(cfg.get("fused_inference", False))
        self.best = None
        self.metrics = StreamingMetrics(model.net.nb_emotions, model.net.device, cfg.get("metrics_top_k", DEFAULT_TOP_K))

    def due(self, step, num_steps):
        return step % self.every == 0 or step == num_steps

    def run(self, step, lr, quiet=False):
        net = self.model.net
        self.metrics.reset()
        averaged = net.store.ema is not None
        with (net.averaged_weights() if averaged else contextlib.nullcontext()):
            for batch in self.model.validation_batches(self.batches):
                self.metrics.update(net.predict(batch, is_training=False, fused=self.fused), batch["labels"])
        res = self.metrics.result()
        _warn_uncounted(res, "validation at step %d" % step)
        with open(os.path.join(self.train_dir, "validation.jsonl"), "a") as f:
            f.write(json.dumps(dict(res, global_step=step, learning_rate=lr, **({"weights": "averaged"} if averaged else {})))
                    + "\n")
        if not quiet:
            print("global step %d: validation accuracy = %.4f, loss = %.4f (%d samples)" % (step, res["accuracy"], res["loss"], res["n"]))
        if self.keep_best and (self.best is None or res["accuracy"] > self.best):
            self.best = res["accuracy"]
            _write_checkpoint(self.model, os.path.join(self.train_dir, "model.best.pt"), step)
            with open(os.path.join(self.train_dir, "best.json"), "w") as f:
                json.dump({"global_step": step, "accuracy": res["accuracy"]}, f)
        return res


def _warn_uncounted(res, what):
    if res["n_nonfinite"] or res["n_bad_label"]:
        print("WARNING: %s: %d rows with non-finite logits and %d rows with a label out of range are not in the metrics"
              % (what, res["n_nonfinite"], res["n_bad_label"]))


def run_training(model, train_dir, num_steps, batch_fn=None, log_every=10, save_interval_secs=600,
                 dropout_mask=None, quiet=False):
    """model: ImageModel / TextModel / DeepSentiment front end (has .net, .config, .dataset)."""
    rank, world = _rank_world()
    resume_from = model.config.get("resume_from")
    if resume_from is not None and os.path.commonpath([os.path.abspath(train_dir), os.path.abspath(resume_from)]) == \
            os.path.abspath(train_dir):
        raise ValueError("config['resume_from'] = %r lies inside train_dir, which is deleted and re-created" % (resume_from,))
    if rank == 0:
        if os.path.exists(train_dir):
            shutil.rmtree(train_dir)           # "Delete old model", :116-118
        os.makedirs(train_dir)
    cfg = model.config
    batch_size, initial_lr, decay = cfg["batch_size"], cfg["initial_lr"], cfg["decay_factor"]
    num_clones = check_clones_config(cfg)      # batch_size is the batch of ONE clone, as in slim
    log_norms = bool(cfg.get("log_gradient_norms", False)) and bool(clip_net_kwargs(cfg))
    # python-2 integer division, :140; under data parallelism one step consumes batch_size * num_clones * world samples
    nb_batches = max(1, model.dataset.num_samples // (batch_size * num_clones * world))
    net = model.net
    validator = Validator(model, train_dir) if rank == 0 and cfg.get("validate_every") is not None else None
    # config['learning_rate_decay_type']: slim's schedules, a function of the steps completed (learning_rate_at); absent: the
    # reference's per-epoch rule below, unchanged
    schedule = check_schedule_config(cfg, model.dataset.num_samples)
    # config['resume_from'] = a checkpoint file: variables, slots, averages and step are restored and steps
    # global_step .. num_steps - 1 are run (the reference never resumes; without the key nothing changes)
    start = 0
    if cfg.get("resume_from") is not None:      # (train_dir has just been emptied: the file lies outside it)
        start = int(load_checkpoint(model, cfg["resume_from"], resume=True))
    epoch = -(-start // nb_batches)      # epochs begun before step `start`
    lr = initial_lr * decay ** max(epoch - 1, 0)
    last_save = time.time()
    loss_val = float("nan")
    t0 = time.time()
    for step in range(start, num_steps):
        if schedule is not None:
            new = float(learning_rate_at(cfg, model.dataset.num_samples, step))
            if rank == 0 and not quiet and (step == start or new != lr):
                print("New learning rate: {0}".format(new))
            lr = new
            if rank == 0:      # one line per step: what the schedule handed to the optimiser
                with open(os.path.join(train_dir, "learning_rate.jsonl"), "a") as f:
                    f.write(json.dumps({"global_step": step, "learning_rate": lr}) + "\n")
        elif step % nb_batches == 0:                                 # :143-147
            lr = initial_lr * decay ** epoch
            if rank == 0 and not quiet:
                print("New learning rate: {0}".format(lr))
            epoch += 1
        model.learning_rate = lr
        batch = batch_fn(step) if batch_fn is not None else model.next_batch(step)
        model.labels = batch["labels"]
        if num_clones > 1:
            net.train_step(batch, lr, dropout_mask=dropout_mask, num_clones=num_clones)
        else:
            net.train_step(batch, lr, dropout_mask=dropout_mask)
        model.logits = net.logits
        if (step + 1) % log_every == 0 or step + 1 == num_steps:
            loss_val = net.total_loss_value()                        # syncs: only on logging steps
            dt = (time.time() - t0) / (log_every if (step + 1) % log_every == 0 else max(1, (step + 1) % log_every))
            if rank == 0 and log_norms:                              # (this step has synchronised already)
                _log_gradient_norms(net, train_dir, step + 1)
            t0 = time.time()
            if rank == 0 and not quiet:
                print("global step %d: loss = %.4f (%.3f sec/step)" % (step + 1, loss_val, dt))
        if validator is not None and validator.due(step + 1, num_steps):
            validator.run(step + 1, lr, quiet=quiet)
        if rank == 0 and time.time() - last_save >= save_interval_secs:
            save_checkpoint(model, train_dir, step + 1)
            last_save = time.time()
    if rank == 0:
        save_checkpoint(model, train_dir, num_steps)
        print("Finished training. Last batch loss {0:.3f}".format(loss_val))
    return loss_val


def load_checkpoint(model, path, averaged=False, resume=False):
    """Restore variables, optimiser slots and step.  resume=True (run_training's config['resume_from']): the file's optimiser
    kind (its 'optimizer' entry; a file without one is adam) must be the net's -- the slots of one kind mean nothing to
    another (slim fails the same way, on missing slot variables): ValueError naming both.  Every other load reads variables,
    and averages when asked for them, and accepts any kind.  A net with moving averages also gets the file's 'moving_averages' (a file
    without them leaves the averages at the variables, where load_state_dict puts them).  averaged=True: the averages are
    loaded IN PLACE OF the trainable variables -- slim's variables_to_restore in eval_image_classifier.py:141-146; a net with
    moving averages then starts them there as well -- and a file without them is a KeyError."""
    ck = torch.load(path, map_location="cpu", weights_only=True)       # never unpickles arbitrary objects
    if resume:
        theirs = ck.get("optimizer", {"optimizer": "adam"})["optimizer"]
        if theirs != model.net.optimizer:
            raise ValueError("%s was written by optimizer %r and cannot resume a run with optimizer %r: the slots of one "
                             "mean nothing to the other" % (path, theirs, model.net.optimizer))
    variables = {k: v.numpy() for k, v in ck["variables"].items()}
    averages = ck.get("moving_averages")
    if averaged:
        if averages is None:
            raise KeyError("%s holds no moving averages: it was not trained with config['moving_average_decay']" % path)
        variables.update({k: v.numpy() for k, v in averages.items()})
    model.net.load_state_dict(variables)
    if averages is not None and not averaged and model.net.store.ema is not None:
        model.net.load_averages_state_dict({k: v.numpy() for k, v in averages.items()})
    model.net.store.m.copy_(ck["adam_m"])
    model.net.store.v.copy_(ck["adam_v"])
    model.net.step = int(ck["global_step"])
    return ck["global_step"]


def run_evaluation(model, checkpoint_dir, log_dir, mode, num_evals, batch_fn=None, quiet=False):
    """What evaluate_* do with slim.evaluation.evaluation_loop + streaming_accuracy
    (im_text_rnn_model.py:171-207): restore the newest checkpoint of `checkpoint_dir`, run `num_evals`
    batches, accumulate accuracy = mean(argmax(logits) == labels).  The reference's loop then waits for
    the next checkpoint forever and writes TensorBoard summaries; here one pass is made, the result is
    returned, printed and appended to <log_dir>/<mode>/accuracy.jsonl.
    As in the reference the graph is built with is_training = (mode == 'train') (:65).  config['fused_inference'] = True:
    the moving-statistics evaluation runs SentimentNet.predict(fused=True) (same logits bit for bit; ignored for mode 'train',
    which keeps batch statistics).  config['eval_metrics'] = True: the batches are accumulated on the device by
    metrics.StreamingMetrics instead of argmax + .item() per batch (one read-back at the end), and its result() -- confusion
    matrix, per-class precision / recall / F1, top-k accuracy, cross-entropy -- is appended with global_step, num_evals and
    mode to <log_dir>/<mode>/metrics.jsonl; the returned accuracy and accuracy.jsonl are what they are without the key."""
    path = latest_checkpoint(checkpoint_dir)
    if path is None:
        raise FileNotFoundError("no checkpoint in %s" % checkpoint_dir)
    # config['moving_average_decay']: score the averaged variables, as slim's eval does when its flag is set
    if getattr(model, "config", {}).get("moving_average_decay") is not None:
        step = load_checkpoint(model, path, averaged=True)
    else:
        step = load_checkpoint(model, path)
    is_training = mode == "train"
    fused = bool(getattr(model, "config", {}).get("fused_inference", False)) and not is_training
    metrics = None
    if getattr(model, "config", {}).get("eval_metrics", False):
        from .metrics import DEFAULT_TOP_K, StreamingMetrics
        metrics = StreamingMetrics(model.net.nb_emotions, model.net.device, model.config.get("metrics_top_k", DEFAULT_TOP_K))
    correct = total = 0
    for i in range(num_evals):
        batch = batch_fn(i) if batch_fn is not None else model.next_batch(10 ** 6 + i)
        logits = model.net.predict(batch, is_training=is_training, fused=fused)
        model.logits, model.labels = logits, batch["labels"]
        if metrics is not None:
            metrics.update(logits, batch["labels"])       # enqueued: nothing is read back until the loop is over
        else:
            correct += int((logits.argmax(dim=1) == batch["labels"]).sum().item())     # streaming_accuracy
        total += int(batch["labels"].shape[0])
    out_dir = os.path.join(log_dir, mode)
    os.makedirs(out_dir, exist_ok=True)
    if metrics is not None:
        res = metrics.result()
        _warn_uncounted(res, "evaluation of step %d" % step)
        # streaming_accuracy's denominator is every row; a row the metrics leave out was not a correct prediction
        correct = sum(row[c] for c, row in enumerate(res["confusion"]))
        with open(os.path.join(out_dir, "metrics.jsonl"), "a") as f:
            f.write(json.dumps(dict(res, global_step=step, num_evals=num_evals, mode=mode)) + "\n")
    acc = correct / max(total, 1)
    with open(os.path.join(out_dir, "accuracy.jsonl"), "a") as f:
        f.write(json.dumps({"global_step": step, "accuracy": acc, "num_evals": num_evals, "mode": mode}) + "\n")
    if not quiet:
        print("global step %d: accuracy = %.4f (%d samples, mode %s)" % (step, acc, total, mode))
    return acc


class SyntheticInput:
    """Mixin: the input side of the reference's model constructors.  If `config['dataset_dir']` holds a
    converted dataset (photos/train_valid_split.txt + tfrecords/tumblr_<mode>_*.tfrecord, the layout of
    datasets/convert_to_dataset.py:117-198) batches are read from it; otherwise they are synthetic.
    config['input_pipeline']: 'host' (default) or 'device' (input_pipeline.DeviceLoader: parallel decode on
    config['input_workers'] threads, default 8, preprocessing on the GPU; the same batches bit for bit).
    config['augment'] (default False): the train-time augmentation of preprocess_for_train (load_batch_with_text's
    is_training=True) on a real dataset -- honoured only once a trainer has called use_augmentation() (train_image_model,
    train_deep_sentiment); evaluate_*, the analyses and class_visualisation always read eval-chain batches, as in the
    reference (im_text_rnn_model.py:291,602).  With config['synthetic'] the key is a ValueError: there is no JPEG to augment.
    config['jpeg_decode']: 'host' (default) or 'device' (compiled Huffman decode + ds_jpeg_reconstruct instead of PIL; the
    same batches bit for bit) -- honoured only with config['input_pipeline'] = 'device'; with the host pipeline the key is
    a ValueError: that pipeline decodes with PIL.
    config['jpeg_entropy']: 'host' (default) or 'device' (the Huffman decode of restart-segmented JPEGs on the GPU too) --
    honoured only with config['jpeg_decode'] = 'device'; with anything else the key is a ValueError.
    config['input_cache']: 'none' (default) or 'device' (every record is decoded once and its pixels stay in an arena of
    config['input_cache_gb'] GB of device memory, a positive number without a default; later passes are assembled from
    there by ds_ragged_gather, the same batches bit for bit) -- honoured only with config['input_pipeline'] = 'device';
    with the host pipeline or config['synthetic'] the key is a ValueError.
    config['eval_metrics'], config['validate_every'], config['validate_batches'], config['keep_best'], config['metrics_top_k']:
    streaming metrics in evaluate_* and validation during train_* (metrics.check_metrics_config lists what each takes;
    a bad value or a key that would do nothing is a ValueError).
    config['feature_cache']: 'none' (default) or 'device' with config['feature_cache_gb'] (a positive number of GB, no
    default): train_image_model / train_deep_sentiment run the frozen tower once per record and then train from Mixed_5b's
    output kept in device memory (feature_cache.py; check_feature_cache_config lists what the key needs and refuses).
    config['num_clones'] = K (default 1): train_* run K clones per rank and step with config['batch_size'] rows each
    (check_clones_config; the trainers call use_clones() before the first batch); evaluate_* and the analyses ignore it.
    config['clip_gradient_norm'], config['clip_global_norm'], config['skip_nonfinite_steps'], config['log_gradient_norms']:
    gradient clipping, the non-finite step guard and gradients.jsonl (clip_net_kwargs).
    config['moving_average_decay'] = d: moving averages of the trained variables in train_*, restored in place of the
    variables by evaluate_* and the analyses (ema_net_kwargs).
    config['optimizer'] ('adam', 'sgd', 'momentum', 'rmsprop') with config['opt_epsilon'], ['momentum'], ['rmsprop_decay'],
    ['adam_beta1'], ['adam_beta2'] (optimizer_net_kwargs) and config['learning_rate_decay_type'] ('fixed', 'exponential',
    'polynomial') with ['learning_rate_decay_factor'], ['num_epochs_per_decay'], ['end_learning_rate'] (check_schedule_config):
    slim's optimiser and learning-rate flags, read by train_* only; config['resume_from'] = a checkpoint file to continue
    from (run_training).
    config['label_smoothing'] = e and config['class_weights'] = [w per emotion]: the other two arguments of
    slim.losses.softmax_cross_entropy, read by train_* only (loss_net_kwargs)."""

    def _init_input(self, config, post_size, vocab_size, nb_emotions, with_images, device):
        from .synthetic import SyntheticDataset
        self._in = (post_size, vocab_size, nb_emotions, with_images, device)
        self.post_ids = self.days = self.labels = None
        self._records = None
        self._augment = False
        self._validation = None
        check_metrics_config(config)
        if config.get("augment", False) and config.get("synthetic", False):
            raise ValueError("config['augment'] needs a real dataset: synthetic batches have no JPEG to augment")
        if config.get("jpeg_decode", "host") not in ("host", "device"):
            raise ValueError("config['jpeg_decode'] must be 'host' or 'device', not %r" % (config["jpeg_decode"],))
        if config.get("jpeg_decode", "host") == "device" and config.get("input_pipeline", "host") != "device":
            raise ValueError("config['jpeg_decode'] = 'device' needs config['input_pipeline'] = 'device': the host pipeline "
                             "decodes with PIL")
        if config.get("jpeg_entropy", "host") not in ("host", "device"):
            raise ValueError("config['jpeg_entropy'] must be 'host' or 'device', not %r" % (config["jpeg_entropy"],))
        if config.get("jpeg_entropy", "host") == "device" and config.get("jpeg_decode", "host") != "device":
            raise ValueError("config['jpeg_entropy'] = 'device' needs config['jpeg_decode'] = 'device': the coefficients go "
                             "to ds_jpeg_reconstruct")
        if config.get("input_cache", "none") not in ("none", "device"):
            raise ValueError("config['input_cache'] must be 'none' or 'device', not %r" % (config["input_cache"],))
        if config.get("input_cache", "none") == "device":
            if config.get("synthetic", False):
                raise ValueError("config['input_cache'] = 'device' needs a real dataset: synthetic batches are not decoded")
            if config.get("input_pipeline", "host") != "device":
                raise ValueError("config['input_cache'] = 'device' needs config['input_pipeline'] = 'device': the arena "
                                 "feeds the device preprocessing")
            gb = config.get("input_cache_gb")
            if isinstance(gb, bool) or not isinstance(gb, (int, float)) or not gb > 0:
                raise ValueError("config['input_cache'] = 'device' needs config['input_cache_gb'], a positive number of GB: "
                                 "there is no default")
        self._feature_cache = None
        check_feature_cache_config(config, with_images)
        ddir = config.get("dataset_dir")
        split = os.path.join(ddir or "", "photos", "train_valid_split.txt")
        if config.get("synthetic", False):
            self.dataset = SyntheticDataset(config.get("num_samples", 50000), nb_emotions)
        elif ddir and os.path.exists(split):
            from .datasets.convert_to_dataset import get_split_with_text
            self.dataset = get_split_with_text(config.get("mode", "train"), ddir)
        else:          # the reference fails in get_split_with_text; never train silently on made-up data
            raise IOError("no converted dataset under config['dataset_dir'] = %r (expected %s).  Set "
                          "config['synthetic'] = True for synthetic batches" % (ddir, split))

    def use_clones(self):
        """Called by the trainers before the first batch: config['num_clones'] takes effect on next_batch()."""
        if self._records is not None:
            raise RuntimeError("use_clones() must precede the first batch")
        self._train_clones = check_clones_config(self.config)
        return self._train_clones

    def use_augmentation(self):
        """Called by the trainers of the models that read images, before the first batch: config['augment'] takes effect."""
        if self._records is not None:
            raise RuntimeError("use_augmentation() must precede the first batch")
        self._augment = bool(self.config.get("augment", False))

    def use_feature_cache(self, rank=None, world=None):
        """Called by the trainers of the models that read images, before the first batch: config['feature_cache'] = 'device'
        takes effect -- next_batch() then serves Mixed_5b features from feature_cache.FeatureCache (built at the first batch,
        i.e. behind the warm start) instead of images.  rank / world: this process's shard (default: the process group's).
        Returns the cache, or None when the key is off."""
        if self._records is not None or self._feature_cache is not None:
            raise RuntimeError("use_feature_cache() must precede the first batch")
        if check_feature_cache_config(self.config, self._in[3]) is not None:
            from .feature_cache import FeatureCache
            self._feature_cache = FeatureCache(self, rank, world)
        return self._feature_cache

    def validation_batches(self, count):
        """The held-out batches of config['validate_every']: the same `count` batches of config['batch_size'] at every call,
        in global order (rank 0, world 1), independent of the training stream, which is not consumed.  Synthetic: the
        batches a single-process evaluate_* reads (seed 10**6 + i), built once and kept on the device.  A real dataset: a
        fresh loader on the 'validation' split -- shuffle=False, the eval preprocessing, the configured 'input_pipeline' /
        'jpeg_*' arms, no 'input_cache', no augmentation -- that is closed when the batches are drawn; it makes one pass at
        most, so a split shorter than count * batch_size gives fewer batches (the ragged tail is dropped as in training)."""
        post_size, vocab, nb, with_images, device = self._in
        bs = self.config["batch_size"]
        if not hasattr(self.dataset, "data_sources"):
            if self._validation is None or len(self._validation) != count:
                self._validation = [to_device(synthetic_batch_numpy(bs, post_size, vocab, nb, seed=10 ** 6 + i,
                                                                    with_images=with_images), device) for i in range(count)]
            yield from self._validation
            return
        from .datasets.convert_to_dataset import get_split_with_text
        from .image_model.im_model import load_batch_with_text
        if self._validation is None:
            self._validation = get_split_with_text("validation", self.config["dataset_dir"])
        if self._validation.num_samples < bs:
            raise ValueError("config['validate_every']: the validation split has %d records, fewer than one batch of %d"
                             % (self._validation.num_samples, bs))
        records = load_batch_with_text(self._validation, bs, shuffle=False, height=224, width=224, is_training=False,
                                       device=device, rank=0, world=1, loop=False, max_token_id=vocab,
                                       num_classes=getattr(self.dataset, "num_classes", nb),
                                       pipeline=self.config.get("input_pipeline", "host"),
                                       workers=self.config.get("input_workers", 8),
                                       jpeg_decode=self.config.get("jpeg_decode", "host"),
                                       jpeg_entropy=self.config.get("jpeg_entropy", "host"), decode_images=with_images)
        try:
            for _, batch in zip(range(count), records):
                yield batch
        finally:
            records.close()

    def next_batch(self, step):
        """The batch of one training step on this rank: config['batch_size'] * config['num_clones'] samples (clone (r, c) is
        slice r * K + c of the global batch); evaluate_* and the analyses never set _train_clones and read batch_size."""
        post_size, vocab, nb, with_images, device = self._in
        rank, world = _rank_world()
        rows = self.config["batch_size"] * getattr(self, "_train_clones", 1)
        if self._feature_cache is not None:                  # config['feature_cache']: features instead of images
            b = self._feature_cache.next_batch()
        elif hasattr(self.dataset, "data_sources"):          # real TFRecords
            if self._records is None:
                from .image_model.im_model import load_batch_with_text
                self._records = load_batch_with_text(self.dataset, rows, height=224, width=224,
                                                     is_training=self._augment, device=device, rank=rank, world=world, max_token_id=vocab,
                                                     num_classes=getattr(self.dataset, "num_classes", nb),
                                                     pipeline=self.config.get("input_pipeline", "host"),
                                                     workers=self.config.get("input_workers", 8),
                                                     jpeg_decode=self.config.get("jpeg_decode", "host"),
                                                     jpeg_entropy=self.config.get("jpeg_entropy", "host"),
                                                     cache=self.config.get("input_cache", "none"),
                                                     cache_bytes=(int(self.config["input_cache_gb"] * 1e9)
                                                                  if self.config.get("input_cache", "none") == "device" else None),
                                                     decode_images=with_images)     # text-only: no JPEG is decoded
            b = next(self._records)
        else:
            gb = rows * world
            b = synthetic_batch_numpy(gb, post_size, vocab, nb, seed=step, with_images=with_images)
            b = to_device(b, device, rank, world)
        self.post_ids, self.days = b["post_ids"], b["days"]
        return b
