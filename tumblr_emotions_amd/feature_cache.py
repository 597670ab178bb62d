"""config['feature_cache'] = 'device': train the head from Mixed_5b's output kept in device memory.

Everything below Mixed_5c is frozen in the reference's fine-tuning job.  With frozen BatchNorm statistics
(config['frozen_bn'] = True), frozen betas (config['trainable_bn_beta'] = False) and no augmentation, Mixed_5b's output is
a pure function of the image and of variables no step writes: [7, 7, 832] fp32, 163 072 bytes an image.  The cache runs
the frozen tower ONCE per image (the build pass, at the first batch), keeps the rows of this rank's shard in one arena
together with the small tensors of a batch, and from then on a training step starts with ONE ds_rows_gather launch that
writes the features into the image engine's Mixed_5b buffer: no file is opened, no JPEG is decoded, no preprocessing and
no frozen layer runs.

A rank trains on ITS OWN shard (records rank, rank + world, ... of the unshuffled file order), shuffled within by a fresh
permutation every pass -- not the loader's order, which shuffles the sources and then the rows of each batch.

The config checks and the sampler are host code and need no device.
"""
import time

import numpy as np

FEATURE_SHAPE = (7, 7, 832)                      # Mixed_5b's output of a 224 x 224 image
FEATURE_FLOATS = 7 * 7 * 832
SMALL_KEYS = ("seq_lens", "labels", "post_ids", "days")      # int64 [N] each, beside texts int64 [N, post_size]


def row_bytes(post_size):
    """Device bytes one cached record takes: the features, the text and the four int64 scalars."""
    return 4 * FEATURE_FLOATS + 8 * int(post_size) + 8 * len(SMALL_KEYS)


def shard_rows(num_samples, rank, world):
    """Records of the unshuffled stream with idx % world == rank."""
    return (int(num_samples) - rank + world - 1) // world if num_samples > rank else 0


def check_feature_cache_config(config, with_images=True):
    """The byte budget of config['feature_cache'] = 'device' (None when the cache is off); needs no device.  ValueError:
    a value other than 'none' / 'device'; a model without an image tower; no config['feature_cache_gb'] (a positive number
    of GB, no default); the cache without config['frozen_bn'] = True and config['trainable_bn_beta'] = False (both make the
    features constants of the run); the cache with config['augment'], config['synthetic'], config['train_all'], a dtype
    other than 'f32' or config['input_cache'] = 'device' (the cache replaces the decoded-pixel arena)."""
    mode = config.get("feature_cache", "none")
    if mode not in ("none", "device"):
        raise ValueError("config['feature_cache'] must be 'none' or 'device', not %r" % (mode,))
    if "trainable_bn_beta" in config and not isinstance(config["trainable_bn_beta"], (bool, np.bool_)):
        raise ValueError("config['trainable_bn_beta'] must be a bool, not %r" % (config["trainable_bn_beta"],))
    if mode == "none":
        return None
    if not with_images:
        raise ValueError("config['feature_cache'] = 'device' needs a model with the image tower")
    gb = config.get("feature_cache_gb")
    if isinstance(gb, (bool, np.bool_)) or not isinstance(gb, (int, float, np.integer, np.floating)) or not gb > 0:
        raise ValueError("config['feature_cache'] = 'device' needs config['feature_cache_gb'], a positive number of GB: "
                         "there is no default")
    if not config.get("frozen_bn", False) or config.get("trainable_bn_beta", True):
        raise ValueError("config['feature_cache'] = 'device' needs config['frozen_bn'] = True and "
                         "config['trainable_bn_beta'] = False: with batch statistics or a trainable beta below Mixed_5c the "
                         "features change from step to step")
    for key in ("augment", "synthetic", "train_all"):
        if config.get(key, False):
            raise ValueError("config['feature_cache'] = 'device' with config[%r]: %s" % (key, {
                "augment": "an augmented image differs from pass to pass",
                "synthetic": "synthetic batches have no records to cache",
                "train_all": "every step would move the layers the features come from"}[key]))
    if config.get("dtype", "f32") != "f32":
        raise ValueError("config['feature_cache'] = 'device' with config['dtype'] = %r: the cache is the fp32 configuration's"
                         % (config["dtype"],))
    if config.get("input_cache", "none") != "none":
        raise ValueError("config['feature_cache'] = 'device' with config['input_cache']: the feature cache replaces the "
                         "decoded-pixel arena (no image is decoded after the build pass)")
    return int(gb * 1e9)


def check_feature_cache_fits(rows, post_size, budget_bytes):
    """ValueError when `rows` records need more than the budget; the message names the GB needed.  No partial mode."""
    need = int(rows) * row_bytes(post_size)
    if need > budget_bytes:
        raise ValueError("config['feature_cache']: %d records need %.3f GB of device memory, config['feature_cache_gb'] "
                         "allows %.3f; there is no partial mode" % (rows, need / 1e9, budget_bytes / 1e9))
    return need


class FeatureSampler:
    """Which rows of its shard a rank trains on, step by step: pass p is a permutation of the shard's rows drawn from
    numpy.random.Generator(PCG64([seed, p, rank])); a step takes the next `rows` entries; every rank makes
    (num_samples // world) // rows steps a pass -- the same count on all ranks, the shorter shard's -- and the rest of the
    permutation is dropped.  Host code."""

    def __init__(self, num_samples, rows, rank=0, world=1, seed=0):
        if not 0 <= rank < world:
            raise ValueError("rank %d outside [0, %d)" % (rank, world))
        if isinstance(rows, (bool, np.bool_)) or rows < 1:
            raise ValueError("rows per step must be a positive int, not %r" % (rows,))
        self.num_samples, self.rows, self.rank, self.world, self.seed = int(num_samples), int(rows), int(rank), int(world), int(seed)
        self.shard = shard_rows(num_samples, rank, world)
        self.steps_per_pass = (self.num_samples // self.world) // self.rows
        if self.steps_per_pass < 1:
            raise ValueError("feature cache: %d records over %d rank(s) give no step of %d rows"
                             % (self.num_samples, self.world, self.rows))

    def permutation(self, p):
        """The shard's rows in the order of pass p, int64 [shard], every value checked to be a row of the shard."""
        perm = np.random.Generator(np.random.PCG64([self.seed, int(p), self.rank])).permutation(self.shard).astype(np.int64)
        if perm.shape != (self.shard,) or (self.shard and (perm.min() < 0 or perm.max() >= self.shard)):
            raise RuntimeError("feature cache: a permutation left the shard")
        return perm

    def locate(self, step):
        """(pass, first entry of the pass's permutation) of training step `step` (0-based)."""
        p, s = divmod(int(step), self.steps_per_pass)
        return p, s * self.rows

    def indices(self, step):
        """The shard rows of training step `step`, int64 [rows]."""
        p, lo = self.locate(step)
        return self.permutation(p)[lo:lo + self.rows]

    def global_indices(self, step):
        """... as indices of the unshuffled record stream (row r of the shard is record rank + r * world)."""
        return self.rank + self.indices(step) * self.world


class FeatureCache:
    """The resident tables of one rank and the batches served from them.  model: an ImageModel / DeepSentiment front end
    (its net, its config, its dataset); rank / world default to the process group's."""

    def __init__(self, model, rank=None, world=None):
        from .training import _rank_world, check_clones_config
        cfg = model.config
        self.model, self.net = model, model.net
        self.budget = check_feature_cache_config(cfg)
        if self.budget is None:
            raise ValueError("config['feature_cache'] is not 'device'")
        r, w = _rank_world()
        self.rank, self.world = (r if rank is None else int(rank)), (w if world is None else int(world))
        self.batch_size, self.clones = int(cfg["batch_size"]), check_clones_config(cfg)
        self.rows = self.batch_size * self.clones
        self.post_size = model._in[0]
        self.sampler = FeatureSampler(model.dataset.num_samples, self.rows, self.rank, self.world, int(cfg.get("seed", 1)))
        check_feature_cache_fits(self.sampler.shard, self.post_size, self.budget)
        self.net.check_features()
        self.tables = None
        self.version = None
        self.served = 0
        self.build_seconds = 0.0
        self._pass = None
        self._perm = None
        self._gather = None
        self._out = None

    # ---- the build pass ---------------------------------------------------------------------------------------------------
    def build(self):
        """One pass over this rank's records in file order through the eval chain and image_features, in batches of
        config['batch_size'] (a ragged last batch is filled up with its last row, so every launch has the training batch's
        plans; only the real rows are kept).  The loader is closed behind it."""
        import torch
        from .image_model.im_model import load_batch_with_text
        t0 = time.time()
        model, cfg, net = self.model, self.model.config, self.net
        post_size, vocab, nb, _, device = model._in
        n, B = self.sampler.shard, self.batch_size
        tables = {"features": torch.empty(n, FEATURE_FLOATS, device=device),
                  "texts": torch.empty(n, post_size, dtype=torch.int64, device=device)}
        for k in SMALL_KEYS:
            tables[k] = torch.empty(n, dtype=torch.int64, device=device)
        # loop=True: the batch that holds the shard's last records is filled up from the next pass (those rows are replaced)
        records = load_batch_with_text(model.dataset, B, shuffle=False, height=224, width=224, is_training=False, device=device,
                                       rank=self.rank, world=self.world, loop=True, max_token_id=vocab,
                                       num_classes=getattr(model.dataset, "num_classes", nb),
                                       pipeline=cfg.get("input_pipeline", "host"), workers=cfg.get("input_workers", 8),
                                       jpeg_decode=cfg.get("jpeg_decode", "host"), jpeg_entropy=cfg.get("jpeg_entropy", "host"))
        try:
            for lo in range(0, n, B):
                b = next(records)
                r = min(B, n - lo)
                images = b["images"]
                if r < B:
                    images = images.clone()
                    images[r:] = images[r - 1]
                f = net.image_features(images)
                tables["features"][lo:lo + r].copy_(f.reshape(B, FEATURE_FLOATS)[:r])
                for k in ("texts",) + SMALL_KEYS:
                    tables[k][lo:lo + r].copy_(b[k][:r])
        finally:
            records.close()
        torch.cuda.synchronize(device)
        self.tables = tables
        self.version = net.image.weights_version
        self._out = {"texts": torch.empty(self.rows, post_size, dtype=torch.int64, device=device)}
        for k in SMALL_KEYS:
            self._out[k] = torch.empty(self.rows, dtype=torch.int64, device=device)
        self._staging = torch.empty((self.rows,) + FEATURE_SHAPE, device=device) if self.clones > 1 else None
        self.build_seconds = time.time() - t0

    # ---- serving ------------------------------------------------------------------------------------------------------------
    def next_batch(self):
        """The batch of the next training step: ONE ds_rows_gather of batch_size * num_clones rows -- the features straight
        into the image engine's Mixed_5b buffer (num_clones = 1; with clones into a staging tensor the clones are sliced
        from), the other tensors into buffers that are reused from step to step."""
        import torch
        from . import ops
        if self.tables is None:
            self.build()
        if self.net.image.weights_version != self.version:
            raise RuntimeError("feature cache: the weights were loaded after the build pass (weights_version %d -> %d); the "
                               "cached features belong to the old ones" % (self.version, self.net.image.weights_version))
        p, lo = self.sampler.locate(self.served)
        if p != self._pass:
            self._perm = torch.from_numpy(self.sampler.permutation(p)).to(self.tables["features"].device)
            self._pass = p
        # the destination is read from the engine at every step: alloc() for another batch size (a predict() during
        # validation) re-allocates the stage buffers
        feat = self._staging if self._staging is not None else self.net.feature_buffer(self.rows)
        if self._gather is None or self._gather_dst != feat.data_ptr():
            pairs = [(self.tables["features"], feat.view(self.rows, FEATURE_FLOATS))]
            pairs += [(self.tables[k], self._out[k]) for k in ("texts",) + SMALL_KEYS]
            self._gather, self._gather_dst = ops.RowsGather(pairs), feat.data_ptr()
        self._gather.run(self._perm[lo:lo + self.rows])
        self.served += 1
        return dict(self._out, features=feat)

    def stats(self):
        n = 0 if self.tables is None else int(self.tables["features"].shape[0])
        return {"rows": n, "bytes": n * row_bytes(self.post_size), "build_seconds": self.build_seconds,
                "passes": 0 if self.tables is None else -(-self.served // self.sampler.steps_per_pass),
                "steps": self.served, "steps_per_pass": self.sampler.steps_per_pass, "rank": self.rank, "world": self.world}
