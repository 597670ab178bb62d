"""Deep Sentiment (joint image + text) model and trainer with the reference's signatures
(image_text_model/im_text_rnn_model.py:38-169)."""
import numpy as np
import torch

from .. import ops
from ..image_model.im_model import get_init_fn
from ..net import SentimentNet
from ..text_model.text_preprocessing import resolve_embedding
from ..feature_cache import check_feature_cache_config
from ..training import SyntheticInput, check_clones_config, clip_net_kwargs, ema_net_kwargs, loss_net_kwargs, optimizer_net_kwargs, \
    check_schedule_config, run_training

_POST_SIZE = 50
_CONFIG = {'mode': 'train',
           'dataset_dir': 'data',
           'text_dir': 'text_model',
           'emb_dir': 'embedding_weights',
           'filename': 'glove.6B.50d.txt',
           'initial_lr': 1e-3,
           'decay_factor': 0.3,
           'batch_size': 64,
           'im_features_size': 256,
           'rnn_size': 1024,
           'final_endpoint': 'Mixed_5c',
           'fc_size': 512}                      # keys verbatim from im_text_rnn_model.py:24-35


class DeepSentiment(SyntheticInput):
    def __init__(self, config, nb_emotions=15, embedding=None, device="cuda", **net_kw):
        self.config = config
        ema_net_kwargs(config)      # (a bad moving_average_decay is refused before anything touches the device)
        if config.get('final_endpoint', 'Mixed_5c') != 'Mixed_5c':
            raise NotImplementedError("final_endpoint must be Mixed_5c")
        self.learning_rate = config['initial_lr']
        post = config.get('post_size', _POST_SIZE)
        # GloVe file -> [V, D] + zero <ukn> row; V and D come from the file (:71-76)
        embedding, vocab, dim, self.word_to_id = resolve_embedding(config, embedding)
        self._init_input(config, post, vocab, nb_emotions, True, device)
        self.nb_emotions = self.dataset.num_classes
        for key in ("train_all", "trainable_embedding", "frozen_bn", "trainable_bn_beta", "sync_bn"):      # optional fine-tuning switches (not in the reference _CONFIG)
            if key in config:
                net_kw.setdefault(key, bool(config[key]))
        if "dtype" in config:
            net_kw.setdefault("dtype", config["dtype"])
        for key, value in clip_net_kwargs(config).items():      # gradient clipping / the non-finite guard (training.py)
            net_kw.setdefault(key, value)
        for key, value in ema_net_kwargs(config).items():      # moving averages of the trained variables (training.py)
            net_kw.setdefault(key, value)
        self.net = SentimentNet(mode="joint", nb_emotions=self.nb_emotions,
                                im_features_size=config['im_features_size'], rnn_size=config['rnn_size'],
                                fc_size=config['fc_size'], vocab_size=vocab, embedding_dim=dim, post_size=post,
                                device=device, **net_kw)
        self.net.initialize(seed=config.get('seed', 1))
        if embedding is not None:
            self.net.store.view("Text/W_embedding").copy_(torch.from_numpy(embedding))
            self.net.store.reset_ema()          # (a trainable table's moving average starts at the assigned table)
        self.embedding = self.net.store.view("Text/W_embedding")
        self.logits = None

    @property
    def concat_features(self):
        """tf.concat([images_features, texts_features], 1) (:95).  The training path never builds it
        (the dense layer reads both halves in place); it is materialised on demand for callers."""
        h = self.net.head
        out = torch.empty(h.B, h.im + h.tx, device=self.net.device)
        ops.copy2d(h.im_feat, h.im_feat.stride(0), out, h.im + h.tx, h.B, h.im)
        ops.copy2d(h.tx_feat, h.tx_feat.stride(0), out[:, h.im:], h.im + h.tx, h.B, h.tx)
        return out


def train_deep_sentiment(checkpoints_dir, train_dir, num_steps, *, config=None, quiet=False):
    """Fine tune the inception model, retraining the last layer (im_text_rnn_model.py:107-169)."""
    config = dict(_CONFIG, **(config or {}))
    check_clones_config(config)      # (before the model is built: a bad num_clones needs no device to be refused)
    check_feature_cache_config(config)
    check_schedule_config(config)
    # slim's optimiser and loss keys reach the net from the trainers only: evaluate_* and the analyses run no optimiser and no loss
    model = DeepSentiment(config, **optimizer_net_kwargs(config), **loss_net_kwargs(config))
    model.use_clones()
    model.use_augmentation()
    model.use_feature_cache()        # config['feature_cache']: built at the first batch, behind the warm start
    init_fn = get_init_fn(checkpoints_dir)
    if init_fn is not None:
        init_fn(model.net)
    return run_training(model, train_dir, num_steps, quiet=quiet)


def evaluate_deep_sentiment(checkpoint_dir, log_dir, mode, num_evals, *, config=None, quiet=False):
    """Accuracy of the newest checkpoint (im_text_rnn_model.py:171-207)."""
    from ..training import run_evaluation
    model = DeepSentiment(dict(_CONFIG, mode=mode, **(config or {})))
    return run_evaluation(model, checkpoint_dir, log_dir, mode, num_evals, quiet=quiet)


# ---- inference-only analyses of the trained joint model (im_text_rnn_model.py:342-575) ----------
# Each one restores the newest checkpoint of `checkpoint_dir` into a validation-mode model (BatchNorm on moving
# statistics, no dropout), runs forward passes on the HIP kernels and writes the same .npy files under `out_dir`
# ('data' in the reference).  `config` overrides _CONFIG as everywhere else in this module.

def _restored_validation_model(checkpoint_dir, config):
    from ..training import latest_checkpoint, load_checkpoint
    model = DeepSentiment(dict(_CONFIG, **dict(config or {}, mode='validation')))
    path = latest_checkpoint(checkpoint_dir)
    if path is None:
        raise FileNotFoundError("no checkpoint in %s" % checkpoint_dir)
    # config['moving_average_decay']: the analyses run on the averaged variables, as slim's eval does when its flag is set
    if model.config.get('moving_average_decay') is not None:
        load_checkpoint(model, path, averaged=True)
    else:
        load_checkpoint(model, path)
    return model


def _forward_batches(model, nb_batches, want_features=False):
    """Yield (logits, labels, days, post_ids[, concat_features]) as numpy arrays for `nb_batches` batches."""
    for i in range(nb_batches):
        batch = model.next_batch(10 ** 6 + i)
        logits = model.net.predict(batch, is_training=False, fused=bool(model.config.get('fused_inference', False)))
        out = [logits.cpu().numpy(), batch["labels"].cpu().numpy(), model.days.cpu().numpy(),
               model.post_ids.cpu().numpy()]
        if want_features:
            out.append(model.concat_features.cpu().numpy())
        yield out


def _save(out_dir, **arrays):
    import os
    os.makedirs(out_dir, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), a)


def correlation_matrix(nb_batches, checkpoint_dir, *, config=None, out_dir='data'):
    """Logits and labels of `nb_batches` validation batches -> posts_logits.npy, posts_labels.npy (:342-376)."""
    model = _restored_validation_model(checkpoint_dir, config)
    rows = list(_forward_batches(model, nb_batches))
    posts_logits = np.vstack([r[0] for r in rows])
    posts_labels = np.hstack([r[1] for r in rows])
    _save(out_dir, posts_logits=posts_logits, posts_labels=posts_labels)
    return posts_logits, posts_labels


def day_of_week_trend(checkpoint_dir, *, config=None, out_dir='data'):
    """Logits, labels, day-of-week and post id of every whole validation batch -> posts_*_week.npy (:531-575)."""
    model = _restored_validation_model(checkpoint_dir, config)
    nb_batches = model.dataset.num_samples // model.config['batch_size']
    rows = list(_forward_batches(model, nb_batches))
    posts_logits = np.vstack([r[0] for r in rows])
    posts_labels, posts_days, posts_ids = (np.hstack([r[k] for r in rows]) for k in (1, 2, 3))
    _save(out_dir, posts_logits_week=posts_logits, posts_labels_week=posts_labels, posts_days_week=posts_days,
          posts_ids_week=posts_ids)
    return posts_logits, posts_labels, posts_days, posts_ids


def outliers_detection(checkpoint_dir, *, config=None, out_dir='data'):
    """Posts whose concatenated image+text feature vector lies farthest (Euclidean) from the validation mean
    (:478-529).  As in the reference the maximum is tracked per batch SLOT k (not globally): slot k keeps the
    largest distance seen at position k of any batch, with that post's id and logits."""
    model = _restored_validation_model(checkpoint_dir, config)
    batch_size = model.config['batch_size']
    nb_batches = model.dataset.num_samples // batch_size
    dense_mean = None
    for i, row in enumerate(_forward_batches(model, nb_batches, want_features=True)):
        m = row[4].mean(axis=0, dtype=np.float64)
        dense_mean = m if dense_mean is None else (i * dense_mean + m) / (i + 1)       # running mean of batch means
    max_norms = np.zeros(batch_size)
    max_post_ids = np.zeros(batch_size)
    max_logits = np.zeros((batch_size, model.dataset.num_classes))
    model._records = None                    # second pass over the same validation stream
    for logits, _, _, post_ids, feats in _forward_batches(model, nb_batches, want_features=True):
        dist = np.linalg.norm(feats - dense_mean, axis=1)
        better = dist > max_norms
        max_norms[better], max_post_ids[better], max_logits[better] = dist[better], post_ids[better], logits[better]
    _save(out_dir, max_norms=max_norms, max_post_ids=max_post_ids, max_logits=max_logits)
    return max_norms, max_post_ids, max_logits


def word_most_relevant(top_words, num_classes, checkpoint_dir, *, config=None, out_dir='data', vocabulary=None):
    """Score single words: a post made of word w alone (sequence length 1, the rest padding) next to an all-zero
    image, through the trained joint model; scores[i] = logits for top_words[i] (:378-475; the reference
    reads an undefined `fc_size` at :436 -- here it comes from the config like everywhere else).
    Returns (scores, vocabulary, word_to_id); `vocabulary` defaults to the GloVe file of the config."""
    model = _restored_validation_model(checkpoint_dir, config)
    assert model.dataset.num_classes == num_classes or num_classes is None
    cfg = model.config
    if vocabulary is None:
        if model.word_to_id is not None:      # the GloVe vocabulary the constructor loaded
            vocabulary = [w for w, _ in sorted(model.word_to_id.items(), key=lambda kv: kv[1]) if w != '<ukn>']
        else:                                 # synthetic run: ids stand for themselves
            vocabulary = [str(i) for i in range(model.net.text.V - 1)]
    word_to_id = dict(zip(vocabulary, range(len(vocabulary))))
    word_to_id['<ukn>'] = len(vocabulary)
    pad = model.net.text.V - 1
    post, batch_size = model.net.text.T, 50                       # the reference hard-codes 50 (:398)
    top_words = np.asarray(top_words, dtype=np.int64)
    scores = []
    dev = model.net.device
    for i in range(len(top_words) // batch_size):                 # a ragged tail is dropped, as in the reference
        texts = np.full((batch_size, post), pad, dtype=np.int64)
        texts[:, 0] = top_words[i * batch_size:(i + 1) * batch_size]
        batch = {"images": torch.zeros(batch_size, 224, 224, 3, device=dev),
                 "texts": torch.from_numpy(texts).to(dev),
                 "seq_lens": torch.ones(batch_size, dtype=torch.int64, device=dev),
                 "labels": torch.zeros(batch_size, dtype=torch.int64, device=dev)}
        scores.append(model.net.predict(batch, is_training=False, fused=bool(cfg.get('fused_inference', False))).cpu().numpy())
    scores = np.vstack(scores) if scores else np.zeros((0, model.dataset.num_classes), np.float32)
    _save(out_dir, top_words_scores=scores, top_words=top_words)
    return scores, vocabulary, word_to_id


# ---- class visualisation: gradient ascent on the input image (im_text_rnn_model.py:209-339) ------------

def deprocess_image(np_image):
    """(:209-210), formula verbatim."""
    return (np_image - 0.5) / 2.0


def _gaussian_filter1d(a, sigma, axis, truncate=4.0):
    """scipy.ndimage.gaussian_filter1d(a, sigma, axis) (order 0, mode 'reflect' = edge sample repeated, truncate 4.0):
    correlation with the normalised kernel exp(-x^2 / (2 sigma^2)), |x| <= int(truncate * sigma + 0.5), in float64."""
    radius = int(truncate * float(sigma) + 0.5)
    x = np.arange(-radius, radius + 1, dtype=np.float64)
    k = np.exp(-0.5 / (float(sigma) ** 2) * x ** 2)
    k /= k.sum()
    a64 = np.asarray(a, dtype=np.float64)
    n = a64.shape[axis]
    pad = [(0, 0)] * a64.ndim
    pad[axis] = (radius, radius)
    p = np.pad(a64, pad, mode='symmetric')
    out = np.zeros_like(a64)
    for i, w in enumerate(k):
        out += w * np.take(p, np.arange(i, i + n), axis=axis)
    return out.astype(np.asarray(a).dtype, copy=False)


def blur_image(np_image, sigma=1):
    """(:212-215): Gaussian blur along axes 1 and 2 (H and W of a [B, H, W, C] batch), scipy-free."""
    np_image = _gaussian_filter1d(np_image, sigma, axis=1)
    np_image = _gaussian_filter1d(np_image, sigma, axis=2)
    return np_image


def class_visualisation(label, learning_rate, checkpoint_dir, *, config=None, num_iterations=500, seed=0, out_dir='data'):
    """Visualise class `label` by gradient ascent on the input image (:217-339) through the newest checkpoint of
    `checkpoint_dir`: the joint model at B = 1 with batch statistics and a fresh dropout draw per iteration, next to a post
    of `post_size` unknown words (the zero embedding row).  J = logit[label] - 0.001 ||x||^2; the step is lr * dJ/dx / ||dJ/dx||
    under a random jitter of up to 16 pixels, then the pixels below the 20th percentile are zeroed and every 10th iteration
    the image is blurred (sigma 0.5).  dlogit/dx comes from SentimentNet.input_gradient (HIP); the post-processing runs in
    NumPy as in the reference.  The start image is preprocess_image of np.random.RandomState(seed).standard_normal((224,
    224, 3)); the jitters are the next draws of that generator.  Writes class_visualisation_<label>.npy to `out_dir` (the
    reference shows the image with matplotlib instead) and returns the final [224, 224, 3] image.
    Deviation: the reference builds an older joint graph (mean-of-embeddings text branch, 128 image features, 6 classes)
    that no checkpoint of its own training path restores; this runs the model that train_deep_sentiment trains."""
    from ..preprocessing.inception_preprocessing import preprocess_image
    import os
    model = _restored_validation_model(checkpoint_dir, config)
    net = model.net
    dev = net.device
    size, post = 224, net.text.T
    blur_every, max_jitter, clip_percentile, l2_reg = 10, 16, 20, 0.001
    rng = np.random.RandomState(seed)
    np_image = preprocess_image(rng.standard_normal((size, size, 3)).astype(np.float32), size, size, is_training=False)[None]
    batch = {"texts": torch.full((1, post), net.text.V - 1, dtype=torch.int64, device=dev),
             "seq_lens": torch.full((1,), post, dtype=torch.int64, device=dev)}
    for i in range(num_iterations):
        ox, oy = rng.randint(-max_jitter, max_jitter + 1, 2)
        np_image = np.roll(np.roll(np_image, ox, 1), oy, 2)
        batch["images"] = torch.from_numpy(np.ascontiguousarray(np_image, dtype=np.float32)).to(dev)
        _, dimg = net.input_gradient(batch, int(label), seed=seed * 1000003 + i)
        grad = dimg.cpu().numpy().astype(np.float32) - np.float32(2.0 * l2_reg) * np_image
        grad = grad / np.linalg.norm(grad)
        np_image = np_image + np.float32(learning_rate) * grad
        np_image = np.roll(np.roll(np_image, -ox, 1), -oy, 2)
        min_norm = np.percentile(np_image, clip_percentile)
        np_image[np_image < min_norm] = 0.0
        if i % blur_every == 0:
            np_image = blur_image(np_image, sigma=0.5)
    os.makedirs(out_dir, exist_ok=True)
    np.save(os.path.join(out_dir, "class_visualisation_%d.npy" % int(label)), np_image[0])
    return np_image[0]


# ---- why did the trained model give this post this emotion? --------------------------------------------------------------

def explain_posts(checkpoint_dir, nb_batches, *, config=None, out_dir='data', method='gradient', steps=32):
    """Explain the PREDICTED class of `nb_batches` validation batches through the newest checkpoint of `checkpoint_dir`, with
    the model as it predicts (BatchNorm on moving statistics, no dropout: SentimentNet.eval_gradients, HIP).
    method 'gradient': gradient x input -- per pixel dlogit/dimage * image, per word sum_d dlogit/dx * x;
    method 'integrated': integrated gradients over `steps` midpoints from a mid-grey image and the zero <ukn> words
    (SentimentNet.integrated_gradients).  Writes under `out_dir` and returns
      saliency_maps.npy      [N, 224, 224]  max over the colour channels of |attribution|
      token_scores.npy       [N, T]         attribution per word, exactly 0 past each post's length
      explained_logits.npy   [N, classes]   the logits that were explained
      explained_post_ids.npy [N]
    Cost of 'integrated': the engines allocate per batch size and layout, so every validation batch re-allocates them twice (the
    forward of predict at `batch_size`, then the interpolation batches at `steps`); choose steps for accuracy, not to match.
    No counterpart in the reference, whose analyses score words in isolation (word_most_relevant) or ascend a class logit from
    noise (class_visualisation)."""
    if method not in ('gradient', 'integrated'):
        raise ValueError("method must be 'gradient' or 'integrated', not %r" % (method,))
    model = _restored_validation_model(checkpoint_dir, config)
    net = model.net
    maps, scores, all_logits, ids = [], [], [], []
    for i in range(nb_batches):
        batch = model.next_batch(10 ** 6 + i)
        batch = {k: batch[k] for k in ("images", "texts", "seq_lens")}
        logits = net.predict(batch, is_training=False).clone()      # (predict hands out the head's own buffer: the calls below rewrite it)
        label = logits.argmax(dim=1)
        if method == 'gradient':
            _, dimg, _, tok = net.eval_gradients(batch, label)
            attr = dimg * batch["images"]
        else:
            attr, tok, _ = net.integrated_gradients(batch, label, steps=steps)
        maps.append(attr.abs().amax(dim=3).cpu().numpy())
        scores.append(tok.cpu().numpy())
        all_logits.append(logits.cpu().numpy())
        ids.append(model.post_ids.cpu().numpy())
    maps, scores, all_logits, ids = np.concatenate(maps), np.concatenate(scores), np.vstack(all_logits), np.hstack(ids)
    _save(out_dir, saliency_maps=maps, token_scores=scores, explained_logits=all_logits, explained_post_ids=ids)
    return maps, scores, all_logits, ids
