"""The Mixed_5b feature cache on the GPU: ds_rows_gather against its host statement, image_features against
the frozen step, the feature step against the image step bit for bit, and the trainers with config['feature_cache'].
B = 4 (one case 8 rows as two clones of 4), 224 x 224 inputs; datasets are generated in tmp_path."""
import os

import numpy as np
import pytest
import torch

import rows_gather_cases as G
from tumblr_emotions_amd import ops

pytestmark = pytest.mark.gpu
FEAT = 7 * 7 * 832
SMALL = dict(rnn_size=32, vocab_size=60, embedding_dim=8, post_size=6)


# ---- 1. the kernel -----------------------------------------------------------------------------------------------------------
def _device_gather(srcs, index, n, src_skew=0, dst_skew=0):
    """ds_rows_gather of uint8 tables on the device; every destination sits between two guard rows of CANARY.  *_skew:
    bytes (a multiple of 4) the table / destination starts past a 256-byte boundary.  Returns the destinations, guards on."""
    pairs, bigs = [], []
    for s in srcs:
        nrows, rb = s.shape
        sbuf = torch.empty(s.size + src_skew, dtype=torch.uint8, device="cuda")
        sv = sbuf[src_skew:].view(nrows, rb)
        sv.copy_(torch.from_numpy(s))
        big = torch.full(((n + 2) * rb + dst_skew,), G.CANARY, dtype=torch.uint8, device="cuda")
        dv = big[dst_skew + rb:dst_skew + (n + 1) * rb].view(n, rb)
        pairs.append((sv, dv))
        bigs.append((big, dst_skew, rb))
    ix = torch.from_numpy(np.ascontiguousarray(index, np.int64)).cuda()
    ops.RowsGather(pairs).run(ix)
    torch.cuda.synchronize()
    return [b[skew:].cpu().numpy().reshape(n + 2, rb) for b, skew, rb in bigs]


def _check(srcs, index, n, **skew):
    want = G.host_reference(srcs, index, n)
    got = _device_gather(srcs, index, n, **skew)
    for w, g in zip(want, got):
        rb = w.shape[1]
        assert np.array_equal(g[1:-1], w), rb
        assert (g[0] == G.CANARY).all() and (g[-1] == G.CANARY).all(), rb      # nothing outside the n rows


@pytest.mark.parametrize("ntables", [1, 3, 8])
def test_kernel_equals_the_host_statement(ntables):
    rng = np.random.default_rng(20 + ntables)
    nrows, n = 13, 9
    index = rng.integers(0, nrows, n)
    index[4] = index[7] = index[1]                       # repeated rows
    index[2], index[6] = -1, nrows                       # ... and two that name nothing: untouched in every table
    rbs = (G.ROW_BYTES * 2)[:ntables] if ntables < 8 else (163072, 400, 8, 8, 8, 8, 4, 20)      # the trainer's six + two
    srcs, _ = G.make_tables(rng, nrows, n, rbs)
    _check(srcs, index, n)


def test_kernel_on_the_four_byte_path_and_past_one_round_of_workgroups():
    rng = np.random.default_rng(31)
    # 400-byte and 163 072-byte rows that start 4 and 8 bytes past a 16-byte boundary: dword accesses, several workgroups
    srcs, _ = G.make_tables(rng, 7, 5, (400, 163072))
    _check(srcs, [6, 0, 3, 3, 1], 5, src_skew=4)
    _check(srcs, [6, 0, 3, 3, 1], 5, dst_skew=8)
    srcs, _ = G.make_tables(rng, 11, 700, (20, 8))        # 3500 dwords: four workgroups of one table beside one of another
    _check(srcs, rng.integers(0, 11, 700), 700)
    # the training shape: 256 feature rows are 2.6 M 16-byte units, more than 2048 workgroups take in one turn (grid stride)
    srcs, _ = G.make_tables(rng, 5, 256, (163072, 400, 8))
    _check(srcs, rng.integers(0, 5, 256), 256)


def test_a_table_beyond_four_gib_is_addressed_in_64_bits():
    """4.5 GiB of untouched memory as a feature table; rows are gathered from its end, above 2**32 bytes: a 32-bit offset
    anywhere in the path reads somewhere else."""
    rb = 4 * FEAT
    nrows = 9 * (1 << 29) // rb
    table = torch.empty(nrows, rb, dtype=torch.uint8, device="cuda")
    rng = np.random.default_rng(3)
    tail = torch.from_numpy(rng.integers(0, 256, (3, rb), dtype=np.uint8)).cuda()
    assert (nrows - 3) * rb > (1 << 32)
    table[nrows - 3:] = tail
    flat = table.view(-1)
    lo = (nrows - 3) * rb - (1 << 32)
    flat[lo:lo + 3 * rb] = 0                                # what a truncated offset would find
    small = torch.arange(nrows, dtype=torch.int64, device="cuda")
    dst = torch.full((4, rb), G.CANARY, dtype=torch.uint8, device="cuda")
    dst8 = torch.full((4,), -1, dtype=torch.int64, device="cuda")
    index = torch.tensor([nrows - 1, nrows - 3, nrows - 2, nrows - 1], device="cuda")
    ops.rows_gather([(table, dst), (small, dst8)], index)
    assert torch.equal(dst, tail[[2, 0, 1, 2]]) and torch.equal(dst8, index)
    del table, flat
    torch.cuda.empty_cache()


# ---- nets and inputs ---------------------------------------------------------------------------------------------------------
def _state(mode, seed=0):
    """Variables under which the signal survives all 57 layers at moving statistics (0, 1): He-normal conv weights, small
    random betas (with the initialiser's 0.01 the activations vanish and every comparison is empty)."""
    net = _make(mode, load=None)
    rng = np.random.default_rng(seed)
    sd = net.state_dict()
    for k, v in sd.items():
        if k.startswith("InceptionV1/") and k.endswith("/weights") and "Logits" not in k:
            sd[k] = rng.normal(0, np.sqrt(2.0 / np.prod(v.shape[:3])), v.shape).astype(np.float32)
        elif k.endswith("/beta"):
            sd[k] = rng.normal(0, 0.1, v.shape).astype(np.float32)
    return sd


def _make(mode, load="cached", **kw):
    from tumblr_emotions_amd.net import SentimentNet
    kw.setdefault("frozen_bn", True)
    kw.setdefault("trainable_bn_beta", False)
    if mode == "joint":
        kw = dict(SMALL, **kw)
    net = SentimentNet(mode=mode, nb_emotions=5, **kw)
    net.initialize(seed=3)
    if load is not None:
        if mode not in _STATES:
            _STATES[mode] = _state(mode)
        net.load_state_dict(_STATES[mode])
    return net


_STATES = {}


@pytest.fixture(scope="module")
def pool():
    """Six posts: images [6, 224, 224, 3] in [-1, 1] (smooth content + noise) and the small tensors; read-only."""
    rng = np.random.default_rng(5)
    yy, xx = np.mgrid[0:224, 0:224]
    imgs = np.stack([np.stack([np.sin(yy / (9.0 + i) + i), np.cos(xx / (13.0 + 2 * i)), ((yy + xx * (i + 1)) % 97) / 48.5 - 1], axis=2)
                     for i in range(6)])
    imgs = np.clip(0.8 * imgs + rng.normal(0, 0.1, imgs.shape), -1, 1).astype(np.float32)
    T = SMALL["post_size"]
    out = {"images": torch.from_numpy(imgs).cuda(),
           "texts": torch.from_numpy(rng.integers(0, SMALL["vocab_size"], (6, T))).cuda(),
           "seq_lens": torch.from_numpy(rng.integers(1, T + 1, 6)).cuda(),
           "labels": torch.from_numpy(rng.integers(0, 5, 6)).cuda()}
    return out


def _rows(pool, idx, keys):
    ix = torch.as_tensor(idx, device="cuda")
    return {k: pool[k][ix].contiguous() for k in keys}


KEYS = {"image": ("images", "labels"), "joint": ("images", "texts", "seq_lens", "labels")}


def _features(net):
    st = net.image._feature_stage()
    return st.out.view(st.out.shape[0], FEAT)


# ---- 2. / 3. the features ----------------------------------------------------------------------------------------------------
def test_features_are_what_the_full_step_leaves_and_no_step_moves_them(pool):
    net = _make("image")
    batch = _rows(pool, [0, 1, 2, 3], KEYS["image"])
    f = net.image_features(batch["images"])
    assert tuple(f.shape) == (4, 7, 7, 832) and f.dtype == torch.float32
    f0 = f.reshape(4, FEAT).clone()
    assert float(f0.abs().max()) > 1e-3 and float((f0 != 0).float().mean()) > 0.2      # a live signal
    theta, step = net.store.theta.clone(), net.step
    assert torch.equal(net.image_features(batch["images"]).reshape(4, FEAT), f0)
    assert torch.equal(net.store.theta, theta) and net.step == step
    net.train_step(batch, 1e-3)
    assert torch.equal(_features(net), f0)                  # the full frozen step left these bits behind Mixed_5b
    for s in (1, 2):
        net.train_step(_rows(pool, [s, 5, 4, 0], KEYS["image"]), 1e-3)
    assert not torch.equal(net.store.theta, theta)
    assert torch.equal(net.image_features(batch["images"]).reshape(4, FEAT), f0)      # nothing the steps train reaches them
    net.train_step(batch, 1e-3)
    assert torch.equal(_features(net), f0)


def test_features_do_not_depend_on_the_position_or_the_companions(pool):
    net = _make("image")
    a = net.image_features(pool["images"][[2, 0, 1, 3]].contiguous()).reshape(4, FEAT)[0].clone()
    b = net.image_features(pool["images"][[5, 4, 3, 2]].contiguous()).reshape(4, FEAT)[3].clone()
    assert float(a.abs().max()) > 1e-3
    assert torch.equal(a, b)


# ---- 4. the step -------------------------------------------------------------------------------------------------------------
def _table(net, pool):
    """A cache-style table [6, 40768] of the pool's features, built in batches of 4 like the cache's build pass."""
    t = torch.empty(6, FEAT, device="cuda")
    t[0:4] = net.image_features(pool["images"][0:4]).reshape(4, FEAT)
    t[2:6] = net.image_features(pool["images"][2:6]).reshape(4, FEAT)
    return t


def _same_state(a, b):
    for x, y in ((a.store.theta, b.store.theta), (a.store.m, b.store.m), (a.store.v, b.store.v), (a.logits, b.logits)):
        assert torch.equal(x, y)
    assert a.total_loss_value() == b.total_loss_value() and a.step == b.step
    sa, sb = a.state_dict(), b.state_dict()
    for k in sa:
        assert np.array_equal(sa[k], sb[k]), k


@pytest.mark.parametrize("mode", ["image", "joint"])
def test_feature_steps_equal_image_steps_bit_for_bit(pool, mode):
    a, b = _make(mode), _make(mode)
    start = a.state_dict()
    table = _table(b, pool)
    for step, idx in enumerate(([0, 1, 2, 3], [3, 0, 5, 1], [5, 4, 3, 2])):      # overlapping images at changing positions
        batch = _rows(pool, idx, KEYS[mode])
        a.train_step(batch, 1e-3)
        fb = dict(batch)
        del fb["images"]
        ix = torch.as_tensor(idx, device="cuda")
        if step != 1:                                        # the trainer's way: gathered straight into the engine's buffer
            fb["features"] = b.feature_buffer(4)
            ops.rows_gather([(table, fb["features"].view(4, FEAT))], ix)
        else:                                                # ... and a tensor of the caller's
            fb["features"] = torch.empty(4, 7, 7, 832, device="cuda")
            ops.rows_gather([(table, fb["features"].view(4, FEAT))], ix)
        b.train_step(fb, 1e-3)
        _same_state(a, b)
    end = a.state_dict()
    moving = [k for k in start if "moving_" in k]
    assert len(moving) == 2 * 57 and all(np.array_equal(start[k], end[k]) for k in moving)
    assert any(not np.array_equal(start[k], end[k]) for k in start if "Mixed_5c" in k and k.endswith("/weights"))


def test_feature_steps_of_two_clones_equal_image_steps(pool):
    a, b = _make("joint"), _make("joint")
    table = _table(b, pool)
    ix = torch.tensor([0, 1, 2, 3, 5, 4, 3, 2], device="cuda")
    batch = _rows(pool, ix.tolist(), KEYS["joint"])
    fb = {k: v for k, v in batch.items() if k != "images"}
    fb["features"] = torch.empty(8, 7, 7, 832, device="cuda")
    ops.rows_gather([(table, fb["features"].view(8, FEAT))], ix)
    for _ in range(2):
        a.train_step(batch, 1e-3, num_clones=2)
        b.train_step(fb, 1e-3, num_clones=2)
        _same_state(a, b)


# ---- 5. the trainers ---------------------------------------------------------------------------------------------------------
def _setup(tmp_path):
    from test_input_pipeline_gpu import _glove, _jpeg_dataset
    root = str(tmp_path / "data")
    ds = _jpeg_dataset(root, n_train=11, n_valid=3)
    ck = str(tmp_path / "warm")
    os.makedirs(ck)
    sd = {k: v for k, v in _state("image").items() if k.startswith("InceptionV1/") and "Logits" not in k}
    np.savez(os.path.join(ck, "inception_v1.npz"), **sd)
    cfg = dict(_glove(root), frozen_bn=True, trainable_bn_beta=False)
    return ds, ck, cfg


def _checkpoint(train_dir, steps):
    from tumblr_emotions_amd.training import latest_checkpoint
    ck = torch.load(latest_checkpoint(train_dir), map_location="cpu", weights_only=True)
    assert ck["global_step"] == steps
    out = {k: v.numpy() for k, v in ck["variables"].items()}
    out.update(adam_m=ck["adam_m"].numpy(), adam_v=ck["adam_v"].numpy())
    return out


def _all_records(ds, keys=("images", "texts", "seq_lens", "labels", "post_ids", "days")):
    from tumblr_emotions_amd.image_model.im_model import load_batch_with_text
    it = load_batch_with_text(ds, batch_size=11, shuffle=False, height=224, width=224, loop=False, max_token_id=100, num_classes=3)
    b = next(it)
    it.close()
    return {k: b[k] for k in keys}


@pytest.fixture
def reads(monkeypatch):
    """Every read_records call, from whichever thread and through either pipeline."""
    from tumblr_emotions_amd.datasets import convert_to_dataset as cd
    from tumblr_emotions_amd.datasets import tfrecord as T
    calls = []
    real = T.read_records

    def counted(path, *a, **k):
        calls.append(path)
        return real(path, *a, **k)

    monkeypatch.setattr(T, "read_records", counted)
    monkeypatch.setattr(cd, "read_records", counted)
    return calls


@pytest.mark.parametrize("rank,world", [(0, 1), (1, 2)])
def test_a_trainer_with_the_cache_equals_image_batches_in_the_cache_s_order(tmp_path, monkeypatch, reads, rank, world):
    from tumblr_emotions_amd import feature_cache as FC
    from tumblr_emotions_amd.image_model.im_model import get_init_fn
    from tumblr_emotions_amd.image_text_model import im_text_rnn_model as M
    from tumblr_emotions_amd.training import run_training
    ds, ck, cfg = _setup(tmp_path)
    made, built = [], []
    init, build = FC.FeatureCache.__init__, FC.FeatureCache.build

    def noted_init(self, *a, **k):
        init(self, *a, **k)
        made.append(self)

    def noted_build(self):
        build(self)
        built.append(len(reads))

    monkeypatch.setattr(FC.FeatureCache, "__init__", noted_init)
    monkeypatch.setattr(FC.FeatureCache, "build", noted_build)
    on = dict(cfg, feature_cache="device", feature_cache_gb=0.01)
    cached_dir, plain_dir = str(tmp_path / "cached"), str(tmp_path / "plain")
    if world == 1:
        loss = M.train_deep_sentiment(ck, cached_dir, 5, config=on, quiet=True)
    else:                                        # the shard of rank 1 of 2, passed explicitly: no process group
        model = M.DeepSentiment(dict(M._CONFIG, **on))
        model.use_clones()
        model.use_augmentation()
        model.use_feature_cache(rank=rank, world=world)
        get_init_fn(ck)(model.net)
        loss = run_training(model, cached_dir, 5, quiet=True)
    cache, = made
    stats = cache.stats()
    n_rank = 11 if world == 1 else 5
    assert stats["rows"] == n_rank and stats["bytes"] == n_rank * (163072 + 400 + 32) and stats["steps"] == 5
    assert stats["passes"] == (3 if world == 1 else 5) and stats["build_seconds"] > 0
    assert built and built[0] >= 2 and len(reads) == built[0]          # no file is opened after the build pass
    # the same records as image batches, in the cache's own index order, through an uncached model
    sampler = FC.FeatureSampler(11, 4, rank, world, seed=1)
    assert np.array_equal(sampler.indices(3), cache.sampler.indices(3))
    everything = _all_records(ds)
    plain = M.DeepSentiment(dict(M._CONFIG, **cfg))
    get_init_fn(ck)(plain.net)

    def batch_fn(step):
        ix = torch.from_numpy(sampler.global_indices(step)).cuda()
        return {k: v[ix].contiguous() for k, v in everything.items()}

    want = run_training(plain, plain_dir, 5, batch_fn=batch_fn, quiet=True)
    assert loss == want and np.isfinite(loss)
    a, b = _checkpoint(cached_dir, 5), _checkpoint(plain_dir, 5)
    assert sorted(a) == sorted(b) and len(a) > 10
    for k in a:
        assert np.array_equal(a[k], b[k]), k


# ---- 6. staleness and refusals -----------------------------------------------------------------------------------------------
def test_a_load_after_the_build_makes_the_next_batch_raise(tmp_path):
    from tumblr_emotions_amd.image_text_model import im_text_rnn_model as M
    from tumblr_emotions_amd.training import load_checkpoint, save_checkpoint
    ds, ck, cfg = _setup(tmp_path)
    model = M.DeepSentiment(dict(M._CONFIG, **dict(cfg, feature_cache="device", feature_cache_gb=0.01)))
    cache = model.use_feature_cache()
    b = model.next_batch(0)
    assert set(b) == {"features", "texts", "seq_lens", "labels", "post_ids", "days"} and "images" not in b
    assert b["features"].data_ptr() == model.net.feature_buffer(4).data_ptr()
    everything = _all_records(ds, ("post_ids", "labels"))
    ix = torch.from_numpy(cache.sampler.global_indices(0)).cuda()
    assert torch.equal(b["post_ids"], everything["post_ids"][ix]) and torch.equal(b["labels"], everything["labels"][ix])
    model.net.train_step(b, 1e-3)
    os.makedirs(str(tmp_path / "t"))
    path = save_checkpoint(model, str(tmp_path / "t"), 1)
    model.next_batch(1)
    load_checkpoint(model, path)
    with pytest.raises(RuntimeError, match="weights were loaded after the build"):
        model.next_batch(2)
    with pytest.raises(RuntimeError, match="precede the first batch"):
        model.use_feature_cache()
    with pytest.raises(ValueError, match="0.002 GB"):          # 11 records: 1.8 MB
        M.DeepSentiment(dict(M._CONFIG, **dict(cfg, feature_cache="device", feature_cache_gb=0.001))).use_feature_cache()


def test_a_predict_of_another_batch_size_between_two_steps_changes_nothing(tmp_path):
    """alloc() for another batch size re-allocates the stage buffers (validation does this): the cache reads its destination
    from the engine at every step, so the run with a predict in between is the run without, bit for bit."""
    from tumblr_emotions_amd.image_text_model import im_text_rnn_model as M
    ds, ck, cfg = _setup(tmp_path)
    on = dict(M._CONFIG, **dict(cfg, feature_cache="device", feature_cache_gb=0.01))
    images = _all_records(ds, ("images", "texts", "seq_lens"))
    nets = []
    for detour in (False, True):
        model = M.DeepSentiment(on)
        model.use_feature_cache()
        for step in range(3):
            model.net.train_step(model.next_batch(step), 1e-3)
            if detour:
                gen = model.net.image.alloc_gen
                model.net.predict({k: v[:2 + step % 2].contiguous() for k, v in images.items()})      # 2 or 3 rows, never the step's 4
                assert model.net.image.alloc_gen > gen
        nets.append(model.net)
    a, b = nets                                   # (b.logits are its last predict's)
    for x in ("theta", "m", "v"):
        assert torch.equal(getattr(a.store, x), getattr(b.store, x)), x
    assert a.total_loss_value() == b.total_loss_value() and a.step == b.step == 3


def test_the_net_refuses_feature_batches_it_cannot_honour(pool):
    from tumblr_emotions_amd.net import SentimentNet
    feats = torch.zeros(4, 7, 7, 832, device="cuda")
    small = {k: v[:4].contiguous() for k, v in pool.items() if k != "images"}
    good = dict(small, features=feats)
    cases = [(_make("image", load=None, frozen_bn=False), good, ValueError),
             (_make("image", load=None, trainable_bn_beta=True), good, ValueError),
             (_make("image", load=None, frozen_bn=False, dtype="bf16"), good, NotImplementedError),
             (_make("image", load=None, frozen_bn=False, train_all=True), good, ValueError),
             (SentimentNet(mode="text", nb_emotions=5, **SMALL), good, ValueError)]
    ok = _make("joint", load=None)
    cases += [(ok, dict(good, images=pool["images"][:4].contiguous()), ValueError),
              (ok, dict(small, features=feats[:3]), ValueError),
              (ok, dict(small, features=feats.view(4, 49, 832)), ValueError),
              (ok, dict(small, features=feats.double()), ValueError),
              (ok, dict(small, features=feats.permute(0, 2, 1, 3)[:, :, :, :]), ValueError),
              (ok, dict(small, features=torch.zeros(4, 7, 7, 1664, device="cuda")[..., ::2]), ValueError)]
    for net, batch, exc in cases:
        theta = net.store.theta.clone()
        for clones in (1, 2):
            with pytest.raises(exc):
                net.train_step(batch, 1e-3, num_clones=clones)
        assert net.step == 0 and torch.equal(net.store.theta, theta)
        if net.mode != "joint":
            with pytest.raises(exc):
                net.image_features(pool["images"][:4]) if net.image is not None else net.check_features()
    with pytest.raises(ValueError):                            # predict stays the image forward
        ok.predict(good)
