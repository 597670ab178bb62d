"""SentimentNet: parameters + engines + one training step, shared by the three reference-shaped
front ends (image_model/im_model.py, text_model/text_embedding.py,
image_text_model/im_text_rnn_model.py in this package).

One step = what `slim.learning.train_step` runs for the reference's train_op
(im_text_rnn_model.py:124-135,152): forward, total loss (CE + L2 of every conv `weights`),
gradients of every trainable variable, BatchNorm moving-average updates, TF Adam.
Data-parallel: gradients are summed over ranks with RCCL all-reduce on two contiguous
buckets of the flat gradient buffer and scaled by 1/world inside the Adam kernel; the L2 term is
applied once, locally, after the reduction (slim/deployment/model_deploy.py:221-223,301-302).
"""
import contextlib
import math

import numpy as np
import torch

from . import ops
from .engine_image import InceptionV1Engine, WEIGHT_DECAY
from .engine_text import JointHeadEngine, TextHeadEngine, TextTowerEngine
from .dp import GradientReducer
from .params import ParamStore

ADAM_B1, ADAM_B2, ADAM_EPS = 0.9, 0.999, 1e-8      # tf.train.AdamOptimizer defaults (:134)


def check_clip_config(clip_gradient_norm=None, clip_global_norm=None):
    """(mode, threshold) of the two clipping arguments; needs no device.  clip_gradient_norm = c: slim's clip_gradient_norms,
    tf.clip_by_norm per variable; clip_global_norm = c: tf.clip_by_global_norm.  ValueError if both are given or c is not a
    finite number > 0 (a bool is not a number)."""
    if clip_gradient_norm is not None and clip_global_norm is not None:
        raise ValueError("clip_gradient_norm and clip_global_norm are mutually exclusive")
    for key, c, mode in (("clip_gradient_norm", clip_gradient_norm, ops.CLIP_PER_VARIABLE),
                         ("clip_global_norm", clip_global_norm, ops.CLIP_GLOBAL)):
        if c is None:
            continue
        if isinstance(c, (bool, np.bool_)) or not isinstance(c, (int, float, np.integer, np.floating)) \
                or not math.isfinite(c) or not c > 0:
            raise ValueError("%s must be a finite number > 0, not %r" % (key, c))
        return mode, float(c)
    return ops.CLIP_NONE, 0.0


def check_ema_config(decay=None):
    """moving_average_decay as a float, or None when it is not given; needs no device.  slim's --moving_average_decay
    (train_image_classifier.py:157): a float with 0 < decay < 1.  ValueError for anything else (a bool is not a number)."""
    if decay is None:
        return None
    if isinstance(decay, (bool, np.bool_)) or not isinstance(decay, (float, np.floating)) or not 0.0 < decay < 1.0:
        raise ValueError("moving_average_decay must be a float with 0 < decay < 1, not %r" % (decay,))
    return float(decay)


def check_loss_config(label_smoothing=None, class_weights=None, nb_emotions=15):
    """(label_smoothing as a float, class_weights as a tuple of floats or None) of the two other arguments of
    slim.losses.softmax_cross_entropy(logits, onehot, weights, label_smoothing); needs no device.  label_smoothing (slim's
    --label_smoothing, train_image_classifier.py:138-139): a finite float with 0 <= label_smoothing < 1 (None: 0).
    class_weights: a sequence of exactly nb_emotions (None: any number of) finite numbers >= 0, not all zero -- the loss
    weight of a row is its label's.  ValueError for anything else (a bool is not a number).  (0.0, None) is the keys-absent case."""
    eps = 0.0
    if label_smoothing is not None:
        x = label_smoothing
        if isinstance(x, (bool, np.bool_)) or not isinstance(x, (int, float, np.integer, np.floating)) \
                or not math.isfinite(x) or not 0.0 <= x < 1.0:
            raise ValueError("label_smoothing must be a finite float with 0 <= label_smoothing < 1, not %r" % (x,))
        eps = float(x)
    cw = None
    if class_weights is not None:
        if isinstance(class_weights, (str, bytes, dict)) or not hasattr(class_weights, "__len__") \
                or not hasattr(class_weights, "__iter__"):
            raise ValueError("class_weights must be a sequence of nb_emotions numbers, not %r" % (class_weights,))
        ws = list(class_weights)
        if nb_emotions is not None and len(ws) != nb_emotions:
            raise ValueError("class_weights must have exactly nb_emotions = %d entries, not %d" % (nb_emotions, len(ws)))
        for w in ws:
            if isinstance(w, (bool, np.bool_)) or not isinstance(w, (int, float, np.integer, np.floating)) \
                    or not math.isfinite(w) or w < 0:
                raise ValueError("class_weights must be finite numbers >= 0, not %r" % (w,))
        if not any(w > 0 for w in ws):
            raise ValueError("class_weights are all zero: no row would count")
        cw = tuple(float(w) for w in ws)
    return eps, cw


OPTIMIZERS = ("adam", "sgd", "momentum", "rmsprop")
_SLIM_OPTIMIZERS_NOT_BUILT = ("adadelta", "adagrad", "ftrl")
# hyper-parameter -> (default, the optimisers that read it); opt_epsilon's default depends on the optimiser (None)
_OPT_HYPER = {"opt_epsilon": (None, ("adam", "rmsprop")), "momentum": (0.9, ("momentum", "rmsprop")),
              "rmsprop_decay": (0.9, ("rmsprop",)), "adam_beta1": (ADAM_B1, ("adam",)), "adam_beta2": (ADAM_B2, ("adam",))}
_OPT_EPSILON = {"adam": ADAM_EPS, "rmsprop": 1.0}


def check_optimizer_config(optimizer="adam", opt_epsilon=None, momentum=0.9, rmsprop_decay=0.9, adam_beta1=ADAM_B1,
                           adam_beta2=ADAM_B2):
    """The optimiser arguments as {'optimizer': name, 'opt_epsilon', 'momentum', 'rmsprop_decay', 'adam_beta1', 'adam_beta2'}
    (floats; a hyper-parameter the optimiser does not read is absent); needs no device.  slim's --optimizer block
    (train_image_classifier.py): 'adam' (the reference's tf.train.AdamOptimizer and the default), 'sgd', 'momentum' (no
    Nesterov), 'rmsprop' (whose momentum is `momentum`).  opt_epsilon=None is 1e-8 for adam (AdamOptimizer's default) and
    1.0 for rmsprop (slim's flag default).  ValueError for an unknown name (the four valid ones are listed), for a value that
    is not a finite number in its range -- 0 <= momentum < 1, 0 < rmsprop_decay < 1, 0 <= adam_beta < 1, opt_epsilon > 0; a
    bool is not a number -- and for a hyper-parameter moved off its default for an optimiser that does not read it (silently
    ignored, a sweep over it would measure nothing).  'adadelta', 'adagrad' and 'ftrl' are a NotImplementedError."""
    if optimizer in _SLIM_OPTIMIZERS_NOT_BUILT:
        raise NotImplementedError("optimizer %r is not implemented (nor are %s); implemented: %s"
                                  % (optimizer, ", ".join(repr(o) for o in _SLIM_OPTIMIZERS_NOT_BUILT if o != optimizer),
                                     ", ".join(OPTIMIZERS)))
    if not isinstance(optimizer, str) or optimizer not in OPTIMIZERS:
        raise ValueError("optimizer must be one of %s, not %r" % (", ".join(repr(o) for o in OPTIMIZERS), optimizer))
    given = {"opt_epsilon": opt_epsilon, "momentum": momentum, "rmsprop_decay": rmsprop_decay, "adam_beta1": adam_beta1,
             "adam_beta2": adam_beta2}
    out = {"optimizer": optimizer}
    for key, x in given.items():
        default, readers = _OPT_HYPER[key]
        if x is None and key == "opt_epsilon":
            if optimizer in readers:
                out[key] = _OPT_EPSILON[optimizer]
            continue
        if isinstance(x, (bool, np.bool_)) or not isinstance(x, (int, float, np.integer, np.floating)) or not math.isfinite(x):
            raise ValueError("%s must be a finite number, not %r" % (key, x))
        if optimizer not in readers:
            if default is None or float(x) != default:
                raise ValueError("%s = %r is given, but optimizer %r does not read it (%s)"
                                 % (key, x, optimizer, " and ".join(repr(o) for o in readers) + " do"))
            continue
        ok = x > 0 if key == "opt_epsilon" else 0 < x < 1 if key == "rmsprop_decay" else 0 <= x < 1
        if not ok:
            raise ValueError("%s must satisfy %s, not %r" % (key, {"opt_epsilon": "opt_epsilon > 0", "rmsprop_decay":
                             "0 < rmsprop_decay < 1"}.get(key, "0 <= %s < 1" % key), x))
        out[key] = float(x)
    return out


def ema_decay(decay, t):
    """decay_t of update t = 1, 2, ... as the fp32 number TF computes with: min(decay, (1 + t) / (10 + t)), what
    tf.train.ExponentialMovingAverage(decay, num_updates=t) uses; the min is taken in double, then rounded once."""
    return np.float32(min(float(decay), (1.0 + t) / (10.0 + t)))


def ema_rate(decay, t):
    """1 - decay_t, formed in fp32 as TF forms it: the factor of (shadow - variable) in update t."""
    return np.float32(1.0) - ema_decay(decay, t)


class SentimentNet:
    def __init__(self, mode="joint", nb_emotions=15, im_features_size=256, rnn_size=512, fc_size=512,
                 vocab_size=10000, embedding_dim=300, post_size=32, image_size=224, dropout_keep_prob=0.8,
                 trainable_bn_beta=True, device="cuda", process_group=None, overlap_comm=True,
                 concurrent_towers=True, train_all=False, trainable_embedding=False, dtype="f32",
                 force_dp_buckets=False, sync_bn=False, frozen_bn=False, clip_gradient_norm=None, clip_global_norm=None,
                 skip_nonfinite_steps=False, moving_average_decay=None, optimizer="adam", opt_epsilon=None, momentum=0.9,
                 rmsprop_decay=0.9, adam_beta1=ADAM_B1, adam_beta2=ADAM_B2, label_smoothing=None, class_weights=None):
        assert mode in ("joint", "image", "text")
        self.dtype = dtype
        # the cross entropy's options (opt-in); refused before anything touches the device.  The logits and
        # dlogits are fp32 in every dtype configuration, so none is refused
        self.label_smoothing, self.class_weights = check_loss_config(label_smoothing, class_weights, nb_emotions)
        # the optimiser (slim's --optimizer); refused before anything touches the device.  opt_epsilon=None:
        # 1e-8 for adam, 1.0 for rmsprop.  Every dtype keeps fp32 variables and steps through the one _optimise below.
        self.opt = check_optimizer_config(optimizer, opt_epsilon, momentum, rmsprop_decay, adam_beta1, adam_beta2)
        self.optimizer = self.opt["optimizer"]
        # adam with AdamOptimizer's defaults: the ds_adam_tf* launches, as before the optimiser could be chosen
        self._reference_adam = self.opt == {"optimizer": "adam", "opt_epsilon": ADAM_EPS, "adam_beta1": ADAM_B1,
                                            "adam_beta2": ADAM_B2}
        # moving averages of the trained variables (opt-in); refused before anything touches the device
        self.ema_decay = check_ema_config(moving_average_decay)
        if self.ema_decay is not None and dtype != "f32":
            raise NotImplementedError("moving_average_decay is implemented for the fp32 configuration, not %r" % dtype)
        # gradient clipping and the non-finite guard (opt-in); refused before anything touches the device
        self.clip_mode, self.clip_norm = check_clip_config(clip_gradient_norm, clip_global_norm)
        self.skip_nonfinite_steps = bool(skip_nonfinite_steps)
        self.clip_active = self.clip_mode != ops.CLIP_NONE or self.skip_nonfinite_steps
        # frozen_bn (opt-in): train_step normalises with the MOVING statistics -- slim.arg_scope([slim.batch_norm],
        # is_training=False) around a tower that otherwise trains (dropout on, the same trainable set, beta's gradient is the
        # plain column sum) -- and never writes them; everything but train_step is that of any other net
        self.frozen_bn = bool(frozen_bn)
        if self.frozen_bn:
            if mode == "text":
                raise ValueError("frozen_bn: mode 'text' has no BatchNorm")
            if sync_bn:
                raise ValueError("frozen_bn with sync_bn: fixed statistics leave nothing to synchronise")
            if dtype != "f32":
                raise NotImplementedError("frozen_bn is implemented for the fp32 configuration, not %r" % dtype)
            if train_all:
                raise NotImplementedError("frozen_bn with train_all is not implemented")
        if not torch.cuda.is_available():
            raise RuntimeError("tumblr_emotions_amd needs an MI355X (HIP) device: the training path has no CPU fallback")
        self.mode, self.nb_emotions, self.device = mode, nb_emotions, torch.device(device)
        self.store = ParamStore(device)
        self.image = self.text = self.head = None
        if mode in ("joint", "image"):
            nc = im_features_size if mode == "joint" else nb_emotions
            self.image = InceptionV1Engine(self.store, nc, image_size, dropout_keep_prob, trainable_bn_beta, device,
                                           train_all=train_all, dtype=dtype)
        if mode in ("joint", "text"):
            self.text = TextTowerEngine(self.store, vocab_size + 1, embedding_dim, rnn_size, post_size, device,
                                        trainable_embedding=trainable_embedding)
        if mode == "joint":
            self.head = JointHeadEngine(self.store, im_features_size, rnn_size, fc_size, nb_emotions, device)
            self.head.image = self.image      # (its parameter gradients ride on the image engine's weight-gradient stream)
        elif mode == "text":
            self.head = TextHeadEngine(self.store, rnn_size, nb_emotions, device)
        self.store.finalize()
        st = self.store
        if self.optimizer == "rmsprop":
            st.v.fill_(1.0)      # RMSPropOptimizer's `rms` slot starts at ones (store.m is its `momentum` slot, at zero)
        self.ema_rate_dev = None
        self._averaged = False       # inside averaged_weights(): theta holds the averages, store.ema the variables
        if self.ema_decay is not None:
            st.enable_ema()
            self.ema_rate_dev = torch.zeros(1, device=self.device)
        # label_smoothing = 0 and no weights: nothing is allocated and the step makes the ds_softmax_ce / ds_slab_epilogue_ce
        # launches it has always made; otherwise the weights live on the device (uploaded once) under one descriptor
        self.class_weights_dev = self.ce_desc = None
        if self.label_smoothing != 0.0 or self.class_weights is not None:
            if self.class_weights is not None:
                self.class_weights_dev = torch.tensor(self.class_weights, dtype=torch.float32, device=self.device)
            self.ce_desc = ops.ce_desc(self.label_smoothing, self.class_weights_dev)
        self.step = 0
        self.frozen_l2_sumsq = 0.0
        self.loss_buf = torch.zeros(1, device=self.device)
        self.l2_buf = torch.zeros(1, device=self.device)
        self.l2_scratch = torch.zeros(256, device=self.device)
        self.lr_t_dev = torch.zeros(1, device=self.device)
        self.seed_dev = torch.zeros(1, dtype=torch.int64, device=self.device)
        self.dlogits = None
        # a step of several clones (train_step(num_clones=K > 1)): allocated by the first one
        self._clone_count = 1
        self.grad_acc = self.clone_loss = self.clone_logits = None
        self._predict_calls = 0
        self.pg = process_group
        from . import streams
        streams.reserve(self.device)
        self.text_stream = streams.get("text", self.device) if (mode == "joint" and concurrent_towers) else None
        if self.text_stream is not None:
            # beside the image tower the persistent LSTM runs four row groups per workgroup: a quarter of the CUs for a
            # longer time instead of a 256-register wave on every SIMD that mostly waits -- the Winograd conv needs
            # whole SIMDs and could not run beside it (joint step 18.5 -> 17.9 ms; text-only keeps 1: shortest sequence).  Round 6:
            # EIGHT -- with the batch sorted by length and the masked steps skipped a workgroup's groups thin out as the steps go,
            # and one workgroup row on H / 16 CUs costs the image tower less than two (13.30 -> 13.24 ms; batches of fewer than
            # eight 32-row groups use as many as they have)
            self.text.seq_rows = 8
        self.reducer = GradientReducer(st.grad, st.n_bucket1, process_group, overlap_comm,
                                       force_buckets=force_dp_buckets)
        self.world = self.reducer.world
        # bucket 1 of the flat gradient is complete once these backward stages have run
        self.reducer.expect(*[n for n, e in (("Mixed_5c", self.image), ("text", self.text), ("head", self.head))
                              if e is not None])
        for e in (self.image, self.text, self.head):
            if e is not None:
                e.reducer = self.reducer
        # sync_bn: BatchNorm over the global batch (off by default: slim's clones -- and the DP parity tests -- keep the
        # statistics per rank, model_deploy.py:353-355)
        self.sync_bn = bool(sync_bn and self.world > 1 and self.image is not None)
        self.sync_bn_requested = bool(sync_bn)      # (train_step(num_clones > 1) refuses the request itself, whatever the world)
        if self.sync_bn:
            if dtype != "f32":
                raise ValueError("sync_bn is implemented for the fp32 configuration")
            self.image.sync_bn, self.image.sync_world, self.image.sync_group = True, self.world, process_group
        self.logits = None
        self.clip_state = None
        if self.clip_active:
            if st.clip_segments.shape[0] == 0:
                raise ValueError("gradient clipping: the model has no trainable variable")
            seg, chunks = st.clip_tables()
            nseg = seg.shape[0]
            # partials (workspace), sumsq [nseg + 1], factors [nseg + 1], flags (non-finite, skip, skipped steps, -)
            self.clip_state = (torch.zeros(chunks.shape[0], dtype=torch.float64, device=self.device),
                               torch.zeros(nseg + 1, dtype=torch.float64, device=self.device),
                               torch.ones(nseg + 1, dtype=torch.float32, device=self.device),
                               torch.zeros(4, dtype=torch.int32, device=self.device))
        self._graph = None           # captured training step (capture_step)
        self._graph_key = None

    # ---- variables --------------------------------------------------------------------------------
    def initialize(self, seed=1):
        """Reference initialisers: conv trunc-normal(0.01) (inception_v1.py:26,59), Logits
        variance-scaling (inception_utils.py:67), tf.get_variable default glorot-uniform for LSTM kernel,
        W_fc, b_fc, W_softmax, b_softmax (im_text_rnn_model.py:89,98-104), zeros for beta / LSTM bias,
        moving mean 0 / variance 1; embedding N(0, 0.4) with a zero <ukn> row (:75)."""
        rng = np.random.RandomState(seed)
        sd = {}

        def trunc(shape, std):
            a = rng.standard_normal(size=shape)
            bad = np.abs(a) > 2
            while bad.any():
                a[bad] = rng.standard_normal(size=int(bad.sum()))
                bad = np.abs(a) > 2
            return (a * std).astype(np.float32)

        def glorot(shape):
            fi, fo = (shape[0], shape[0]) if len(shape) == 1 else (int(np.prod(shape[:-1])), shape[-1])
            lim = math.sqrt(6.0 / (fi + fo))
            return rng.uniform(-lim, lim, size=shape).astype(np.float32)

        for e in self.store.entries.values():
            n, shp = e.name, e.shape
            if n.endswith("/weights") and "/Logits/" in n:
                v = trunc(shp, math.sqrt(1.3 * 2.0 / (shp[0] * shp[1] * shp[2])))
            elif n.endswith("/weights"):
                v = trunc(shp, 0.01)
                if shp[2] == 4 and shp[0] == 7:
                    v[:, :, 3, :] = 0                      # stem: the zero-padded 4th input channel
            elif n.endswith("moving_variance"):
                v = np.ones(shp, np.float32)
            elif n.endswith("beta") or n.endswith("moving_mean") or n.endswith("/biases") or n.endswith("cell/bias"):
                v = np.zeros(shp, np.float32)
            elif n == "Text/W_embedding":
                v = rng.normal(0, 0.4, size=shp).astype(np.float32)
                v[-1] = 0
            else:
                v = glorot(shp)
            self.store.view(n).copy_(torch.from_numpy(v))
        self.after_load()

    def load_state_dict(self, sd, strict=True):
        """sd uses the reference's TF variable names; the stem's [7,7,3,64] weights are zero-padded to 4 inputs."""
        sd = dict(sd)
        k = "InceptionV1/Conv2d_1a_7x7/weights"
        if k in sd and np.asarray(sd[k]).shape[2] == 3:
            w = np.zeros((7, 7, 4, 64), np.float32)
            w[:, :, :3, :] = np.asarray(sd[k])
            sd[k] = w
        seen = self.store.load_state_dict(sd, strict)
        self.after_load()
        return seen

    def state_dict(self):
        sd = self.store.state_dict()
        k = "InceptionV1/Conv2d_1a_7x7/weights"
        if k in sd:
            sd[k] = sd[k][:, :, :3, :].copy()
        return sd

    def grads_state_dict(self):
        torch.cuda.synchronize()
        sd = self.store.state_dict(grads=True)
        k = "InceptionV1/Conv2d_1a_7x7/weights"
        if k in sd:                      # train_all: drop the zero-padded 4th input channel of the stem
            sd[k] = sd[k][:, :, :3, :].copy()
        return sd

    # ---- moving averages of the trained variables -----------------------------------
    def _need_averages(self, what):
        if self.store.ema is None:
            raise RuntimeError("%s needs moving_average_decay: this net keeps no moving averages" % what)

    def averages_state_dict(self):
        """{tf_name: array} of the moving averages of the TRAINABLE variables, split and trimmed as state_dict() does (the
        block-input 1x1 convs under their own names, the stem with 3 inputs).  Inside averaged_weights() too these are the
        averages, not the variables.  load_averages_state_dict is the inverse."""
        self._need_averages("averages_state_dict()")
        torch.cuda.synchronize()
        if self._averaged:      # (exchanged: theta holds them)
            names = self._trainable_tf_names()
            sd = {n: v for n, v in self.store.state_dict().items() if n in names}
        else:
            sd = self.store.state_dict(which="ema")
        k ="InceptionV1/Conv2d_1a_7x7/weights"
        if k in sd:
            sd[k] = sd[k][:, :, :3, :].copy()
        return sd

    def _trainable_tf_names(self):
        out = set()
        for e in self.store.entries.values():
            if e.trainable:
                out.update([n for (n, _, _) in e.columns] if e.columns else [e.name])
        return out

    def load_averages_state_dict(self, sd, strict=True):
        """Moving averages from {tf_name: array} (what averages_state_dict returns; a checkpoint's 'moving_averages')."""
        self._need_averages("load_averages_state_dict()")
        if self._averaged:
            raise RuntimeError("load_averages_state_dict inside averaged_weights()")
        sd = dict(sd)
        k = "InceptionV1/Conv2d_1a_7x7/weights"
        if k in sd and k in self._trainable_tf_names() and np.asarray(sd[k]).shape[2] == 3:
            w = np.zeros((7, 7, 4, 64), np.float32)
            w[:, :, :3, :] = np.asarray(sd[k])
            sd[k] = w
        return self.store.load_state_dict(sd, strict, which="ema")

    @contextlib.contextmanager
    def averaged_weights(self):
        """with net.averaged_weights(): predict, forward, eval_gradients, integrated_gradients, input_gradient and
        image_features see the moving averages in place of the trainable variables (what slim's eval restores with
        variables_to_restore).  The CONTENTS of store.theta and store.ema are exchanged -- the engines hold addresses into
        theta, which stay -- and exchanged back on exit, so both buffers get their old bits back.  Around each exchange what
        an optimiser step invalidates is invalidated (the fused forward's prepared statistics) and nothing more: the frozen
        filters' prepared copies and a captured step stay valid.  train_step, capture_step and a nested averaged_weights()
        raise RuntimeError inside."""
        self._need_averages("averaged_weights()")
        if self._averaged:
            raise RuntimeError("averaged_weights() is already entered: it does not nest")
        self._exchange_averages()
        self._averaged = True
        try:
            yield self
        finally:
            self._exchange_averages()
            self._averaged = False

    def _exchange_averages(self):
        st = self.store
        tmp = st.theta.clone()
        st.theta.copy_(st.ema)
        st.ema.copy_(tmp)
        if self.image is not None:
            self.image.invalidate_fused()

    def after_load(self):
        """L2 of the frozen conv weights is a constant of the run: sum it once.  The moving averages start at the variables."""
        self.store.reset_ema()
        tot = 0.0
        for e in self.store.entries.values():
            if (not e.trainable) and e.name.endswith("/weights"):
                ops.sumsq(self.store.view(e.name), e.numel, self.l2_scratch, self.l2_buf)
                tot += float(self.l2_buf.item())
        self.frozen_l2_sumsq = tot
        if self.image is not None:
            self.image.weights_version += 1      # Winograd-transformed copies of the frozen filters are stale
        # ... and so is a captured step: the frozen layers' weight transforms are not part of the capture
        if getattr(self, "_graph", None) is not None:
            self.release_graph()

    # ---- forward / loss ---------------------------------------------------------------------------
    def _towers(self, batch, dropout_mask, seed, fused=False):
        """(im, tx): the image tower enqueued on the current stream and the text tower -- in the joint model ~130
        launch-latency-bound kernels (LSTM steps) -- beside it on its own HIP stream, forked and joined with events."""
        im = tx = None
        side = self.text_stream if (self.image is not None and self.text is not None) else None
        if side is not None:
            main = torch.cuda.current_stream()
            inputs_ready = torch.cuda.Event()
            inputs_ready.record(main)
        if self.image is not None and "features" in batch:      # Mixed_5b's output instead of images (check_feature_batch)
            B = batch["features"].shape[0]
            buf = self.image.feature_buffer(B)
            if batch["features"].data_ptr() != buf.data_ptr():      # (the feature cache gathers straight into the buffer)
                buf.copy_(batch["features"])
            im = self.image.forward_from_features(B, dropout_mask, seed)
        elif self.image is not None:
            im = self.image.forward(batch["images"], dropout_mask, seed, fused=fused)
        if side is not None:
            side.wait_event(inputs_ready)          # NOT wait_stream: the image tower is already enqueued on main
            if self.image.text_gate is not None and self.image.text_gate_event is not None:
                side.wait_event(self.image.text_gate_event)      # (A/B: start behind a stage of the image tower)
            with torch.cuda.stream(side):
                tx = self.text.forward(batch["texts"], batch["seq_lens"])
            main.wait_stream(side)
        elif self.text is not None:
            tx = self.text.forward(batch["texts"], batch["seq_lens"])
        return im, tx

    def forward(self, batch, dropout_mask=None, seed=0, fused=False):
        """batch: dict with device tensors images [B,224,224,3] f32, texts [B,T] i64, seq_lens [B] i64.  Returns the logits
        buffer of the engines (nothing here is recorded by autograd: gradients come from train_step, input_gradient and
        eval_gradients, which drive the engines' backward passes themselves)."""
        im, tx = self._towers(batch, dropout_mask, seed, fused)
        if self.mode == "image":
            self.logits = im
        elif self.mode == "text":
            self.logits = self.head.forward(tx)
        else:
            self.logits = self.head.forward(im, tx)
        return self.logits

    def predict(self, batch, is_training=False, seed=None, fused=False):
        """Forward only (evaluate_*): is_training=False -> BatchNorm moving statistics, no dropout;
        is_training=True reproduces the reference's evaluation on mode='train' (batch statistics and
        dropout stay on, im_text_rnn_model.py:65) but never touches the moving averages.
        fused=True (fp32, is_training=False): the image tower applies BatchNorm + ReLU inside its conv launches and prepares
        the moving statistics once per weight version -- the same logits bit for bit, fewer passes over the activations
        (fused_report() lists the layers that kept the separate pass).  The text tower and the heads are
        unchanged."""
        if fused and is_training:
            raise ValueError("predict(fused=True) is the moving-statistics forward: is_training must be False")
        if fused and self.dtype != "f32":
            raise NotImplementedError("predict(fused=True) is implemented for the fp32 configuration, not %r" % self.dtype)
        if self.image is not None:
            self.image.training, self.image.update_moving = is_training, False
        # evaluation on mode='train' keeps dropout on: every call draws a fresh mask (a fixed seed would apply
        # the identical mask to every evaluation batch)
        self._predict_calls += 1
        seed = (1 << 40) + self._predict_calls if seed is None else seed
        try:
            with torch.no_grad():
                return self.forward(batch, None, seed=self._rank_seed(seed), fused=bool(fused))
        finally:
            if self.image is not None:
                self.image.training, self.image.update_moving = True, True

    def fused_report(self):
        """[(layer key, reason)]: the conv layers that kept conv -> BatchNorm-apply in the last predict(fused=True)."""
        return [] if self.image is None else self.image.fused_report()

    def input_gradient(self, batch, target, *, is_training=True, dropout_mask=None, seed=None):
        """(logits, dimages): the forward pass of predict(is_training=True) and the exact gradient of
        J = sum_b sum_k target[b, k] logits[b, k] with respect to batch['images'] ([B, H, W, 3], BatchNorm's batch-statistics
        terms included: what tf.gradients gives in the reference's class_visualisation, im_text_rnn_model.py:217-339).
        target: an int label (every sample), a [B] int64 label tensor (one-hot) or a [B, nb_emotions] float tensor.  In the
        joint model the text tower runs forward only: its features are constants of J.  Variables, moving statistics, Adam
        slots and `step` are not touched; no weight gradient is formed and nothing is all-reduced (this rank's gradient)."""
        if self.image is None:
            raise ValueError("input_gradient needs the image tower (mode 'image' or 'joint'), not mode %r" % self.mode)
        if self.dtype != "f32":
            raise NotImplementedError("input_gradient is implemented for the fp32 configuration, not %r" % self.dtype)
        if not is_training:
            raise NotImplementedError("input_gradient differentiates batch-statistics BatchNorm (is_training=True) only")
        images = batch["images"]
        B = images.shape[0]
        target = self._target_matrix(target, B)
        self._input_grad_calls = getattr(self, "_input_grad_calls", 0) + 1
        seed = (1 << 41) + self._input_grad_calls if seed is None else seed
        eng = self.image
        sync = eng.sync_bn
        eng.training, eng.update_moving, eng.sync_bn = True, False, False
        try:
            with torch.no_grad():
                im = eng.forward(images, dropout_mask, self._rank_seed(seed), input_grad=True)
                if self.mode == "image":
                    logits = im.clone()
                    dimg = eng.input_backward(target, torch.empty(images.shape, device=self.device))
                else:
                    tx = self.text.forward(batch["texts"], batch["seq_lens"])
                    logits = self.head.forward(im, tx).clone()
                    d_im = self.head.input_backward(target)
                    dimg = eng.input_backward(d_im, torch.empty(images.shape, device=self.device))
        finally:
            eng.training, eng.update_moving, eng.sync_bn = True, True, sync
        return logits, dimg

    def _target_matrix(self, target, B):
        """The three target forms of input_gradient / eval_gradients as a float32 [B, nb_emotions] matrix on the device."""
        nc = self.nb_emotions
        if isinstance(target, (int, np.integer)):
            target = torch.full((B,), int(target), dtype=torch.int64, device=self.device)
        target = torch.as_tensor(target, device=self.device)
        if target.dtype in (torch.int32, torch.int64) and target.dim() == 1 and target.shape[0] == B:
            if bool(((target < 0) | (target >= nc)).any()):
                raise ValueError("target labels must lie in [0, %d)" % nc)
            target = torch.nn.functional.one_hot(target.long(), nc).float()
        elif target.is_floating_point() and tuple(target.shape) == (B, nc):
            target = target.float().contiguous()
        else:
            raise ValueError("target must be an int, a [B] label tensor or a [B, %d] float tensor" % nc)
        return target

    def eval_gradients(self, batch, target, *, text_scale=None):
        """(logits, dimages, dwords, token_scores) of the TRAINED model's prediction: the forward pass of
        predict(is_training=False) -- BatchNorm with its moving statistics, no dropout; the logits are that call's, bit for
        bit -- and the exact gradient of J = sum_b sum_k target[b, k] logits[b, k] with respect to
          * batch['images']: dimages [B, H, W, 3] (None in mode 'text'),
          * the embedded words x[b, t, :] = table[texts[b, t]]: dwords [B, T, D], zero at t >= seq_lens[b] (None in mode 'image'),
        plus token_scores [B, T] = sum_d dwords * x (gradient x input; exactly 0 past each post's length).  target: as for
        input_gradient.  text_scale (optional float32 [B]): the embedded words of sample b are text_scale[b] * table[id] (the
        straight path from the zero <ukn> row that integrated_gradients walks); dwords / token_scores are then with respect to
        those scaled words.  fp32 only.
        With fixed statistics every sample is independent and BatchNorm's backward is pointwise: no reduction, no finalize
        (DESIGN.md 7.5).  Variables, Adam slots, `step`, moving statistics and statistics pivots are not touched, no weight
        gradient is formed, nothing is all-reduced; the next train_step is that of a net that never called this."""
        if self.dtype != "f32":
            raise NotImplementedError("eval_gradients is implemented for the fp32 configuration, not %r" % self.dtype)
        B = (batch["images"] if self.image is not None else batch["texts"]).shape[0]
        target = self._target_matrix(target, B)
        if text_scale is not None:
            if self.text is None:
                raise ValueError("text_scale needs the text tower (mode 'text' or 'joint')")
            text_scale = torch.as_tensor(text_scale, dtype=torch.float32, device=self.device).contiguous()
            if tuple(text_scale.shape) != (B,):
                raise ValueError("text_scale must be a [B] float tensor")
        eng = self.image
        dimg = dwords = scores = None
        if eng is not None:
            eng.training, eng.update_moving = False, False
        try:
            with torch.no_grad():
                im = tx = None
                if eng is not None:
                    images = batch["images"]
                    im = eng.forward(images, None, 0, input_grad=True)
                if self.text is not None:
                    tx = self.text.forward(batch["texts"], batch["seq_lens"], scale=text_scale)
                if self.mode == "image":
                    logits = im.clone()
                    dimg = eng.input_backward(target, torch.empty(images.shape, device=self.device), eval_mode=True)
                elif self.mode == "text":
                    logits = self.head.forward(tx).clone()
                    dwords, scores = self.text.input_backward(self.head.input_backward(target))
                else:
                    logits = self.head.forward(im, tx).clone()
                    d_im, d_tx = self.head.input_backward(target, with_text=True)
                    dimg = eng.input_backward(d_im, torch.empty(images.shape, device=self.device), eval_mode=True)
                    dwords, scores = self.text.input_backward(d_tx)
        finally:
            if eng is not None:
                eng.training, eng.update_moving = True, True
                eng.invalidate_fused()      # (this pass left its own rstd / shift where the fused pass keeps its prepared ones)
        return logits, dimg, dwords, scores

    def integrated_gradients(self, batch, target, *, steps=32, image_baseline=None):
        """Integrated gradients of the trained model's logit J (target as for eval_gradients), one post at a time: the `steps`
        midpoints alpha_k = (k + 0.5) / steps of the straight path from the baseline go through eval_gradients as ONE batch of
        `steps` samples (exact: with moving statistics the samples are independent).  Image path x0 + alpha (x - x0), x0 =
        image_baseline ([H, W, 3] or [B, H, W, 3]; default zeros, the preprocessed mid-grey); word path alpha * x, from the zero
        <ukn> row.  Returns (image_attr [B, H, W, 3] or None, token_attr [B, T] or None, f_x - f_x0 [B]): attribution =
        (x - x0) * mean gradient, summed over D for the words; f_x - f_x0 is what the attributions sum to as steps grows.
        Every call inside runs at batch size `steps`, so the engines are allocated once for the whole method."""
        if self.dtype != "f32":
            raise NotImplementedError("integrated_gradients is implemented for the fp32 configuration, not %r" % self.dtype)
        steps = int(steps)
        if steps < 1:
            raise ValueError("steps must be >= 1")
        has_im, has_tx = self.image is not None, self.text is not None
        B = (batch["images"] if has_im else batch["texts"]).shape[0]
        target = self._target_matrix(target, B)
        alpha = (torch.arange(steps, device=self.device, dtype=torch.float32) + 0.5) / steps
        im_attr = torch.empty(batch["images"].shape, device=self.device) if has_im else None
        tok_attr = torch.empty(batch["texts"].shape, device=self.device) if has_tx else None
        if has_im:
            x_all = batch["images"]
            x0_all = torch.zeros_like(x_all) if image_baseline is None else \
                torch.as_tensor(image_baseline, dtype=torch.float32, device=self.device).expand_as(x_all).contiguous()
        for b in range(B):
            sub = {}
            if has_im:
                x, x0 = x_all[b:b + 1], x0_all[b:b + 1]
                sub["images"] = (x0 + alpha.view(steps, 1, 1, 1) * (x - x0)).contiguous()
            if has_tx:
                sub["texts"] = batch["texts"][b:b + 1].expand(steps, -1).contiguous()
                sub["seq_lens"] = batch["seq_lens"][b:b + 1].expand(steps).contiguous()
            _, dimg, dwords, _ = self.eval_gradients(sub, target[b:b + 1].expand(steps, -1).contiguous(),
                                                    text_scale=alpha if has_tx else None)
            if has_im:
                im_attr[b] = (x_all[b] - x0_all[b]) * dimg.mean(0)
            if has_tx:
                words = self.text.table[batch["texts"][b]]          # [T, D]: the embedded words of the post itself
                tok_attr[b] = (words * dwords.mean(0)).sum(-1)
        # f(x) - f(x0): the 2 B end points, in batches of `steps` samples (the batch size the engines are allocated for: another
        # one would re-allocate every tower); a short last batch is filled up with its own last sample
        idx = torch.arange(2 * B, device=self.device)
        f = torch.empty(2 * B, device=self.device)
        for i in range(0, 2 * B, steps):
            take = idx[i:i + steps]
            pad = torch.cat([take, take[-1:].expand(steps - take.shape[0])])
            post, at_x = pad % B, pad >= B                  # samples [0, B): the baselines, [B, 2 B): the posts themselves
            ends = {}
            if has_im:
                ends["images"] = torch.where(at_x.view(-1, 1, 1, 1), x_all[post], x0_all[post]).contiguous()
            if has_tx:
                ends["texts"], ends["seq_lens"] = batch["texts"][post].contiguous(), batch["seq_lens"][post].contiguous()
            lg, _, _, _ = self.eval_gradients(ends, target[post].contiguous(), text_scale=at_x.float() if has_tx else None)
            f[take] = (lg * target[post]).sum(1)[:take.shape[0]]
        delta = f[B:] - f[:B]
        return im_attr, tok_attr, delta

    def total_loss_value(self):
        """Host value of slim.losses.get_total_loss(): CE + sum_conv wd*||W||^2/2 (syncs).  Since this read
        synchronises anyway it also checks the persistent LSTM's error words (ds_lstm_seq_status) and raises if a
        launch since the last read timed out on a workgroup hand-off -- its results, and this loss, are invalid."""
        reg = 0.0
        if self.store.n_l2 > 0 or self.frozen_l2_sumsq:
            reg = 0.5 * WEIGHT_DECAY * (self.frozen_l2_sumsq + float(self.l2_buf.item()))
        if self._clone_count > 1:      # slim's total loss of this rank's clones: the mean of their cross-entropies
            ce = 0.0
            for x in self.clone_loss.cpu().tolist():      # summed in clone order, in double
                ce += x
            ce /= self._clone_count
        else:
            ce = float(self.loss_buf.item())
        loss = ce + reg
        self.check_status()
        return loss

    def check_status(self):
        """Device-side failure words of the step kernels (today: the persistent LSTM's hand-off timeouts)."""
        if self.text is not None:
            torch.cuda.synchronize(self.device)
            self.text.check_status()

    def _rank_seed(self, seed):
        return int(seed) * 4096 + self.reducer.rank

    # ---- Mixed_5b features in place of images ---------------------------------------
    def check_features(self):
        """What the feature passes need of the net; raises before anything is enqueued or counted."""
        if self.image is None:
            raise ValueError("features need the image tower (mode 'image' or 'joint'), not mode %r" % self.mode)
        if self.dtype != "f32":
            raise NotImplementedError("features are implemented for the fp32 configuration, not %r" % self.dtype)
        if self.image.train_all:
            raise ValueError("features with train_all: every step would move the layers the features come from")
        if not self.frozen_bn:
            raise ValueError("features need frozen_bn=True: batch statistics tie a sample's features to its batch")
        self.image.check_features()

    def check_feature_batch(self, batch):
        """A train_step batch that carries 'features' ([B, 7, 7, 832] fp32, contiguous, on the device) in place of 'images'."""
        self.check_features()
        if "images" in batch:
            raise ValueError("a batch carries either 'images' or 'features', not both")
        f = batch["features"]
        st = self.image._feature_stage()
        if not torch.is_tensor(f) or f.dtype != torch.float32 or f.dim() != 4 or tuple(f.shape[1:]) != (st.H, st.W, st.C) \
                or f.shape[0] != batch["labels"].shape[0] or not f.is_contiguous() or not f.is_cuda:
            raise ValueError("features must be a contiguous float32 device tensor [B, %d, %d, %d] with one row per label"
                             % (st.H, st.W, st.C))

    def image_features(self, images):
        """Mixed_5b's output [B, 7, 7, 832] fp32 for `images` ([B, 224, 224, 3] as for train_step): the frozen-statistics
        training forward stopped behind Mixed_5b -- the bits a frozen train_step on the same images leaves there, whatever
        the other images of the batch are.  A view of the engine's stage buffer: copy it before the next pass.  Variables,
        moving statistics, Adam slots and `step` are not touched."""
        self.check_features()
        with torch.no_grad():
            return self.image.forward_features(images)

    def feature_buffer(self, B):
        """The buffer a feature batch of B rows is read from (Mixed_5b's output of the image engine): a batch whose
        'features' IS this tensor is used in place, any other is copied into it.  Ask at every step, keep nothing."""
        self.check_features()
        return self.image.feature_buffer(B)

    # ---- one training step -----------------------------------------------------------------------
    def train_step(self, batch, lr, dropout_mask=None, seed=None, num_clones=1, after_clone=None):
        """One optimiser step on `batch`.  num_clones = K > 1: the step of K of slim's in-graph clones on this device, run back
        to back -- clone c is rows [c B/K, (c+1) B/K) of every tensor of `batch` (and of `dropout_mask`), has
        its own BatchNorm batch statistics and the dropout stream of virtual rank rank*K + c; the clone gradients are summed in
        clone order by ds_grad_accumulate, all-reduced once, and Adam runs once with grad_scale 1 / (world * K); the L2 term is
        counted once, the moving statistics are clone 0's, `step` advances once.  `logits` then holds all B rows in order and
        total_loss_value() the mean of the K cross-entropies + the L2 term.  after_clone(c), a test and diagnostic hook, is
        called once clone c's backward pass and accumulation are enqueued, before clone c + 1 starts.  num_clones = 1 is the
        plain step, launch for launch.
        A batch may carry 'features' ([B, 7, 7, 832] fp32: Mixed_5b's output, image_features()) in place of 'images' on a
        frozen_bn net with trainable_bn_beta=False: the image tower then runs from Mixed_5c on (check_feature_batch lists what
        is refused, before anything is enqueued or counted); the step is the image step's, bit for bit."""
        if "features" in batch:
            self.check_feature_batch(batch)
        if self._averaged:
            raise RuntimeError("train_step inside averaged_weights(): the variables are exchanged for their moving averages")
        if type(num_clones) is not int or num_clones != 1:
            return self._train_step_clones(batch, lr, dropout_mask, seed, num_clones, after_clone)
        self._clone_count = 1
        st = self.store
        lr_t = self._begin_step(lr)
        # dropout stream: one seed per (step, rank) -- ranks must not share a mask pattern across their shards
        seed = self._rank_seed(self.step) if seed is None else seed
        if self._graph is not None:
            if self._graph_key == self._batch_key(batch, dropout_mask):
                # replay of the captured step: only the two per-step scalars change, and they live on the device
                self.seed_dev.fill_(seed)
                self.lr_t_dev.fill_(lr_t)
                if self.ema_rate_dev is not None:
                    self.ema_rate_dev.fill_(float(ema_rate(self.ema_decay, self.step)))
                self._graph.replay()
                return self.loss_buf.view(())
            if self._graph_key[-2:] != self._batch_key(batch, dropout_mask)[-2:]:
                self.release_graph()     # buffers re-allocated or weights reloaded since the capture: the graph is stale
        self.reducer.begin_step()      # engines call reducer.stage_done(...): bucket 1 is all-reduced under the backward
        self._step_body(batch, dropout_mask, seed, self.loss_buf)
        grad_scale = self.reducer.finish()
        self._optimise(grad_scale, lr_t)
        return self.loss_buf.view(())

    def _optimise(self, grad_scale, lr_t, lr_t_dev=None, ema_rate_dev=None):
        """The optimiser behind a step's gradients (all-reduced and clone-summed in store.grad): one ds_adam_tf launch -- or,
        with clip_gradient_norm / clip_global_norm / skip_nonfinite_steps, the norm launches (ds_grad_norms) and the Adam launch
        that reads their factors and skip flag from device memory (ds_adam_tf_clipped).  Nothing synchronises; store.grad is
        only read.  Under data parallelism every rank reduces the same summed buffer with the same kernels, so the ranks
        clip and skip alike.
        With moving_average_decay the Adam launch is its _ema twin (ds_adam_tf_ema / ds_adam_tf_clipped_ema): the same bits in
        theta, m and v, and store.ema moved towards the new theta by the rate of step `self.step` (ema_rate_dev: read from
        device memory instead, the captured step) in the same pass.
        The one place that chooses the optimiser: any other `optimizer`, or adam with its own betas / epsilon, is the same
        sequence with ONE ds_opt_step in place of the Adam launch (lr_t: _begin_step's step scalar; store.m / store.v are
        slot0 / slot1)."""
        st = self.store
        rate = 0.0 if self.ema_decay is None else float(ema_rate(self.ema_decay, max(self.step, 1)))
        if not self._reference_adam:
            kw = {}
            if self.clip_active:
                seg, chunks = st.clip_tables()
                partials, sumsq, factors, flags = self.clip_state
                ops.grad_norms(st.theta, st.grad, st.n_trainable_padded, st.n_l2, WEIGHT_DECAY, grad_scale, seg, chunks,
                               self.clip_mode, self.clip_norm, self.skip_nonfinite_steps, partials, sumsq, factors, flags)
                kw.update(segments=seg, chunks=chunks, factors=factors, flags=flags)
            if self.ema_decay is not None:
                kw.update(shadow=st.ema, ema_rate=rate, ema_rate_dev=ema_rate_dev)
            o = self.opt
            ops.opt_step(ops.OPT_KINDS[self.optimizer], st.theta, st.grad, st.m, st.v, st.n_trainable_padded, st.n_l2,
                         WEIGHT_DECAY, grad_scale, lr_t, b1=o.get("adam_beta1", 0.0), b2=o.get("adam_beta2", 0.0),
                         eps=o.get("opt_epsilon", 0.0), momentum=o.get("momentum", 0.0), rho=o.get("rmsprop_decay", 0.0),
                         lr_dev=lr_t_dev, **kw)
            return
        if not self.clip_active:
            if self.ema_decay is not None:
                ops.adam_tf_ema(st.theta, st.grad, st.m, st.v, st.ema, st.n_trainable_padded, st.n_l2, WEIGHT_DECAY, grad_scale,
                                lr_t, rate, ADAM_B1, ADAM_B2, ADAM_EPS, lr_t_dev=lr_t_dev, ema_rate_dev=ema_rate_dev)
                return
            ops.adam_tf(st.theta, st.grad, st.m, st.v, st.n_trainable_padded, st.n_l2, WEIGHT_DECAY, grad_scale, lr_t,
                        ADAM_B1, ADAM_B2, ADAM_EPS, lr_t_dev=lr_t_dev)
            return
        seg, chunks = st.clip_tables()
        partials, sumsq, factors, flags = self.clip_state
        ops.grad_norms(st.theta, st.grad, st.n_trainable_padded, st.n_l2, WEIGHT_DECAY, grad_scale, seg, chunks, self.clip_mode,
                       self.clip_norm, self.skip_nonfinite_steps, partials, sumsq, factors, flags)
        if self.ema_decay is not None:
            ops.adam_tf_clipped_ema(st.theta, st.grad, st.m, st.v, st.ema, st.n_trainable_padded, st.n_l2, WEIGHT_DECAY,
                                    grad_scale, lr_t, rate, ADAM_B1, ADAM_B2, ADAM_EPS, seg, chunks, factors, flags,
                                    lr_t_dev=lr_t_dev, ema_rate_dev=ema_rate_dev)
            return
        ops.adam_tf_clipped(st.theta, st.grad, st.m, st.v, st.n_trainable_padded, st.n_l2, WEIGHT_DECAY, grad_scale, lr_t,
                            ADAM_B1, ADAM_B2, ADAM_EPS, seg, chunks, factors, flags, lr_t_dev=lr_t_dev)

    def grad_norms(self):
        """Gradient norms of the last step, one synchronising read of what ds_grad_norms left on the device: {tf_name: the
        variable's ||g_eff||_2 BEFORE clipping} (g_eff = what compute_gradients(total_loss) returns: summed over ranks and
        clones, scaled by 1 / (world * clones), L2 term included; the three block-input 1x1 convs of a fused tensor each
        under their own name) plus 'global_norm', 'factor' (clip_global_norm: the one factor applied) or 'factors'
        ({tf_name: factor}; all 1.0 under skip_nonfinite_steps alone), 'nonfinite' (some norm of that step was NaN / Inf) and
        'skipped_steps' (steps the guard has skipped so far).  Needs one of clip_gradient_norm, clip_global_norm,
        skip_nonfinite_steps: a net without them runs no norm launch (skip_nonfinite_steps=True is the one that changes no
        finite step)."""
        if not self.clip_active:
            raise RuntimeError("grad_norms() needs clip_gradient_norm, clip_global_norm or skip_nonfinite_steps: this net "
                               "runs no gradient-norm launch")
        torch.cuda.synchronize(self.device)
        _, sumsq, factors, flags = self.clip_state
        sumsq, factors, flags = sumsq.cpu().numpy(), factors.cpu().numpy(), flags.cpu().numpy()
        names = self.store.clip_names
        out = {n: float(math.sqrt(x)) if x >= 0 else float("nan") for n, x in zip(names, sumsq[:-1])}
        tot = float(sumsq[-1])
        out["global_norm"] = math.sqrt(tot) if tot >= 0 else float("nan")
        if self.clip_mode == ops.CLIP_GLOBAL:
            out["factor"] = float(factors[-1])
        else:
            out["factors"] = {n: float(f) for n, f in zip(names, factors[:-1])}
        out["nonfinite"] = bool(flags[0])
        out["skipped_steps"] = int(flags[2])
        return out

    def _begin_step(self, lr):
        """Count the step and return the optimiser's step scalar (what lr_t_dev carries in a captured step): Adam's
        bias-corrected lr_t = lr sqrt(1 - b2^t) / (1 - b1^t) with the configured betas, the learning rate for the others."""
        self.step += 1
        if self.image is not None:
            self.image.invalidate_fused()      # beta and the moving statistics move: predict(fused=True) prepares them again
        if self.optimizer != "adam":
            return lr
        b1, b2 = self.opt["adam_beta1"], self.opt["adam_beta2"]
        return lr * math.sqrt(1.0 - b2 ** self.step) / (1.0 - b1 ** self.step)

    def _l2_term(self):
        """sum(w^2) over the trainable weights under the L2 regulariser, before the update.  Only total_loss_value() reads it."""
        st = self.store
        ops.sumsq(st.theta, st.n_l2, self.l2_scratch, self.l2_buf)

    def _step_body(self, batch, dropout_mask, seed, loss_out, l2=True):
        """Everything a step enqueues between the batch and the optimiser -- the towers, the head, the cross entropy (into
        loss_out) with its gradient, the L2 term (l2=False: not this time), the backward passes -- with the engines driven
        directly.  The eager step, every clone of a step of several and the captured step are this one sequence."""
        labels = batch["labels"]
        B, C_ = labels.shape[0], self.nb_emotions
        if self.dlogits is None or self.dlogits.shape[0] != B:
            self.dlogits = torch.empty(B, C_, device=self.device)
        if self.frozen_bn:     # the statistics mode of this forward and backward: moving statistics, read-only
            self.image.frozen_step = True
        try:
            im, tx = self._towers(batch, dropout_mask, seed)
            ce_done = False
            if self.mode == "image":
                logits = im
            elif self.mode == "text":
                logits = self.head.forward(tx)
            else:
                # ce_done: the cross entropy and its gradient from the launch that combines the W_softmax GEMM (the same bits);
                # the head is asked about the plans of THIS batch size (none yet: forward builds them, one ds_softmax_ce below)
                self.head.alloc(B)
                ce_done = self.head.grouped() and self.head.ce_fused()
                ce = None
                if ce_done:      # (with label_smoothing / class_weights: the descriptor rides along)
                    ce = (labels, loss_out, self.dlogits) + (() if self.ce_desc is None else (self.ce_desc,))
                logits = self.head.forward(im, tx, ce=ce)
            self.logits = logits
            if not ce_done:
                if self.ce_desc is None:
                    ops.softmax_ce(logits, labels, B, C_, 1.0, None, loss_out, self.dlogits)
                else:      # label_smoothing / class_weights: the same launch with the descriptor (read at enqueue time)
                    ops.softmax_ce_opts(self.ce_desc, logits, labels, B, C_, 1.0, None, loss_out, self.dlogits)
            # The L2 term, on the pre-update weights: with the grouped head chain the engine whose backward() runs first runs it
            # behind its parameter gradients on the weight-gradient stream (joined before the optimiser); otherwise here
            job = self._l2_term if (l2 and self.store.n_l2 > 0) else None
            grouped = self.head.grouped() if self.mode == "joint" else (self.mode == "image" and self.image.head_group)
            if job is not None and not grouped:
                job()
                job = None
            if self.mode == "image":
                self.image.backward(self.dlogits, side_job=job)
            elif self.mode == "text":
                self.text.backward(self.head.backward(self.dlogits))
            else:
                # (the head may leave its parameter gradients on the image engine's weight-gradient stream: image.backward joins it)
                d_im, d_tx = self.head.backward(self.dlogits, side_job=job)
                side = self.text_stream
                if side is not None:              # BPTT next to the Inception backward; the (short) text backward first, so that
                    main = torch.cuda.current_stream()      # bucket 1 of the gradient is complete right after Mixed_5c
                    side.wait_stream(main)
                    with torch.cuda.stream(side):
                        self.text.backward(d_tx)
                    self.image.backward(d_im)
                    main.wait_stream(side)
                else:
                    self.text.backward(d_tx)
                    self.image.backward(d_im)
        finally:
            if self.frozen_bn:
                self.image.frozen_step = False

    # ---- one training step of several clones ---------------------------------------------------------
    def check_clones(self, num_clones, batch_rows=None, seed=None):
        """The combinations train_step(num_clones=K > 1) refuses, before anything is enqueued or counted."""
        K = num_clones
        if isinstance(K, bool) or not isinstance(K, (int, np.integer)) or K < 1:
            raise ValueError("num_clones must be a positive int, not %r" % (K,))
        K = int(K)
        if K == 1:
            return K
        if self.sync_bn_requested:
            raise ValueError("num_clones = %d with sync_bn: clones have their own BatchNorm statistics by definition" % K)
        if self.dtype != "f32":
            raise NotImplementedError("num_clones = %d with dtype %r: clones are implemented for the fp32 configuration"
                                      % (K, self.dtype))
        if self._graph is not None:
            raise NotImplementedError("num_clones = %d with a captured step: release_graph() first, a step of several "
                                      "clones is not captured" % K)
        if seed is not None:
            raise ValueError("num_clones = %d with an explicit seed: every clone draws its own dropout stream" % K)
        if K * self.world > 4096:
            raise ValueError("num_clones * world = %d exceeds the 4096 dropout streams of a step" % (K * self.world))
        if batch_rows is not None and batch_rows % K != 0:
            raise ValueError("num_clones = %d does not divide the batch of %d rows" % (K, batch_rows))
        return K

    @staticmethod
    def _clone_rows(t, lo, hi):
        """Rows [lo, hi) of a batch tensor: a view where it keeps the 16-byte alignment the kernels load with."""
        v = t[lo:hi]
        return v if v.data_ptr() % 16 == 0 and v.is_contiguous() else v.clone(memory_format=torch.contiguous_format)

    def _train_step_clones(self, batch, lr, dropout_mask, seed, num_clones, after_clone):
        B = int(batch["labels"].shape[0])
        K = self.check_clones(num_clones, B, seed)
        if K == 1:
            return self.train_step(batch, lr, dropout_mask=dropout_mask, seed=seed)
        st = self.store
        b = B // K
        nc = self.nb_emotions
        if self.grad_acc is None:
            self.grad_acc = torch.zeros_like(st.grad)
        if self.clone_loss is None or self.clone_loss.shape[0] != K:
            self.clone_loss = torch.zeros(K, device=self.device)
        if self.clone_logits is None or tuple(self.clone_logits.shape) != (B, nc):
            self.clone_logits = torch.empty(B, nc, device=self.device)
        lr_t = self._begin_step(lr)
        try:
            self.reducer.begin_step(defer=True)      # store.grad is complete only after the last accumulation
            for c in range(K):
                lo, hi = c * b, (c + 1) * b
                sub = {k: self._clone_rows(v, lo, hi) for k, v in batch.items()}
                mask = None if dropout_mask is None else self._clone_rows(dropout_mask, lo, hi)
                # the dropout stream of virtual rank rank * K + c: the numbering of a (K * world)-rank run
                clone_seed = int(self.step) * 4096 + self.reducer.rank * K + c
                if self.image is not None:
                    self.image.update_moving = c == 0      # the moving averages are clone 0's (model_deploy.py:353-355)
                self._step_body(sub, mask, clone_seed, self.clone_loss[c:c + 1], l2=c == 0)      # (the L2 term once)
                self.clone_logits[lo:hi].copy_(self.logits)
                ops.grad_accumulate(self.grad_acc, st.grad, st.n_trainable_padded, 0 if c == 0 else (2 if c == K - 1 else 1))
                if after_clone is not None:
                    after_clone(c)
        finally:
            if self.image is not None:
                self.image.update_moving = True
        self.reducer.finish()
        self.logits = self.clone_logits
        self._clone_count = K
        self._optimise(1.0 / (self.world * K), lr_t)
        return self.clone_loss

    # ---- the same step as one hipGraph ---------------------------------------------------------------
    def _batch_key(self, batch, dropout_mask):
        # the engines' allocation generation is part of the key: alloc() for another batch size (a predict() in
        # between) frees every buffer the captured kernels point at, so the old graph must never be replayed
        gen = tuple(getattr(e, "alloc_gen", 0) for e in (self.image, self.text, self.head) if e is not None)
        wv = self.image.weights_version if self.image is not None else 0
        return tuple(sorted((k, v.data_ptr(), tuple(v.shape)) for k, v in batch.items())) + (
            None if dropout_mask is None else dropout_mask.data_ptr(), gen, wv)

    def capture_step(self, batch, dropout_mask=None, num_clones=1):
        """Capture one whole training step on `batch`'s tensors (static addresses: refill them in place between
        steps) into a hipGraph; later train_step calls with the same tensors replay it -- one graph launch instead
        of ~900 kernel launches, which is what bounds the step below ~64 samples per GPU.  Per-step scalars (Adam's
        lr_t, the dropout seed) are read from device memory.  Single rank only: with data parallelism the RCCL
        all-reduce stays outside a graph and the eager step is used."""
        if self._averaged:
            raise RuntimeError("capture_step inside averaged_weights(): the variables are exchanged for their moving averages")
        if type(num_clones) is not int or num_clones != 1:
            if self.check_clones(num_clones) > 1:
                raise NotImplementedError("capture_step with num_clones = %d: a step of several clones is not captured"
                                          % num_clones)
        if self.frozen_bn:
            raise NotImplementedError("capture_step is not implemented for a frozen_bn net")
        if self.reducer.active:
            return False
        st = self.store
        # eager warm-up (allocates every buffer, builds every plan) on a snapshot of the optimiser state, so that
        # capturing has no side effect on the variables, the Adam slots or the BatchNorm moving statistics
        state = (st.theta, st.m, st.v, st.frozen) + (() if self.clip_state is None else (self.clip_state[3],)) + \
            (() if st.ema is None else (st.ema,))      # (the warm-up's lr is 0, but its step would still move the averages)
        keep = [b.clone() for b in state]      # (the guard's count of skipped steps is state too)
        if self.image is not None and self.image.B != batch["images"].shape[0]:
            self.image.alloc(batch["images"].shape[0])
        if self.image is not None:
            # the small-batch default (a side stream per branch chain, side_mode 0) is for eager launches: hipStreamEndCapture
            # of this ROCm (7.2) segfaults on the joint step captured with three chains joined per block (B = 32, real dims),
            # and a replayed graph gains nothing from it (4.07 ms with one side stream) -- whatever side_mode says, a captured
            # step keeps ONE side stream (0: three joined side streams break hipStreamEndCapture; 2: slower as a graph, 3.95 vs
            # 3.78 ms); release_graph() puts the eager arrangement back
            im = self.image
            im.one_side_stream = im.side_arrangement(im.side_mode, im.B, im.dtype, capturing=True)
        # ... and of the BatchNorm pivots (each layer's previous batch mean), so that the first replayed step rounds
        # exactly like the eager step it replaces
        pivots = [] if self.image is None else [l.mean for l in self.image.layers]
        keep_pivots = [m.clone() for m in pivots]
        self.train_step(batch, 0.0, dropout_mask)
        self.step -= 1
        for b, k in zip(state, keep):
            b.copy_(k)
        for m, k in zip(pivots, keep_pivots):
            m.copy_(k)
        if self.image is not None:
            self.image.seed_dev = self.seed_dev
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            self._step_body(batch, dropout_mask, 0, self.loss_buf)      # (the seed of a replay is seed_dev's)
            self._optimise(1.0, 0.0, lr_t_dev=self.lr_t_dev, ema_rate_dev=self.ema_rate_dev)
        self._graph, self._graph_key = g, self._batch_key(batch, dropout_mask)
        return True

    def release_graph(self):
        """Drop the captured step (also called by after_load(): a load changes weights the capture baked in)."""
        self._graph = self._graph_key = None
        if self.image is not None:
            self.image.seed_dev = None       # eager steps and predict() take the host seed again
            im = self.image
            if im.B is not None:      # capture_step narrowed it to one side stream: back to what alloc chooses for this batch size
                im.one_side_stream = im.side_arrangement(im.side_mode, im.B, im.dtype)
