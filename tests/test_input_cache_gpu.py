"""cache='device' on the GPU: ds_ragged_gather against its host statement (the grid of test_input_cache_cpu.py, a record
that does not fit, an arena beyond 2**32 bytes), and the loader with the cache on against the host pipeline -- every key,
bitwise, in the same order, over three passes and a bit: both chains, all three decode arms, an arena too small, two
ranks, other sizes and formats, the errors, the lifetime, one front-end run.  Datasets are generated in tmp_path."""
import ctypes as C
import gc
import io
import os
import threading

import numpy as np
import pytest
import torch

import gather_cases as G
from test_input_pipeline_gpu import KEYS, _glove, _jpeg_dataset, _png_dataset
from tumblr_emotions_amd import _lib, ops
from tumblr_emotions_amd.datasets import convert_to_dataset as cd
from tumblr_emotions_amd.datasets import dataset_utils as du
from tumblr_emotions_amd.datasets import tfrecord as T
from tumblr_emotions_amd.image_model.im_model import load_batch_with_text

pytestmark = pytest.mark.gpu
MB = 1 << 20


# ---- the kernel ------------------------------------------------------------------------------------------------------------------
def _run_device(case, desc=None, check=True):
    big = torch.from_numpy(case.guarded()).cuda()
    out = big[G.GUARD:G.GUARD + case.nout]
    arena = torch.from_numpy(case.arena).cuda()
    spill = None if case.spill is None else torch.from_numpy(case.spill).cuda()
    if check:
        ops.ragged_gather(arena, spill, case.desc, out)
    else:                                         # past ops' check: the library directly
        d = torch.from_numpy(np.ascontiguousarray(desc).view(np.uint8)).cuda()
        rc = _lib.load().ds_ragged_gather(C.c_void_p(arena.data_ptr()), arena.numel(), None if spill is None else C.c_void_p(spill.data_ptr()),
                                          0 if spill is None else spill.numel(), C.c_void_p(d.data_ptr()), int(desc.size),
                                          C.c_void_p(out.data_ptr()), out.numel(), None)
        assert rc == 0
    torch.cuda.synchronize()
    return big.cpu().numpy()


def test_kernel_equals_the_host_statement_on_the_grid_guards_included():
    cases = G.cases()
    for i, c in enumerate(cases):
        want = G.run_host(c)
        assert np.array_equal(want, c.want)
        assert np.array_equal(_run_device(c), want), (i, c.desc)


def test_a_record_that_does_not_fit_is_left_alone_and_its_neighbours_are_copied():
    c = [c for c in G.cases() if c.desc.size == 7 and c.spill is not None][0]
    for field, value in (("src_offset", 1 << 40), ("out_offset", c.nout), ("src", 3), ("pitch", 0), ("height", 1 << 30)):
        desc = c.desc.copy()
        desc[field][3] = value
        want = c.want.copy()
        at, n = G.GUARD + int(c.desc["out_offset"][3]), int(c.desc["height"][3]) * int(c.desc["width"][3]) * 3
        want[at:at + n] = G.pattern(want.size)[at:at + n]
        assert np.array_equal(_run_device(c, desc, check=False), want), field


def test_an_arena_beyond_four_gib_is_addressed_in_64_bits():
    """4.5 GiB of untouched memory with one 17 x 9 image just above 2**32 bytes: a 32-bit offset anywhere in the path reads
    somewhere else."""
    arena = torch.empty(9 * (1 << 29), dtype=torch.uint8, device="cuda")
    rng = np.random.RandomState(3)
    img = rng.randint(0, 256, (17, 9, 3)).astype(np.uint8)
    off = (1 << 32) + 4096 + 16
    arena[off:off + img.size] = torch.from_numpy(img.reshape(-1)).cuda()
    arena[off - (1 << 32):off - (1 << 32) + img.size] = 0       # what a truncated offset would find
    desc = np.zeros(2, ops.gather_desc_dtype())
    desc[0] = (off, 0, 0, 27, 0, 0, 17, 9)
    desc[1] = (off, 460, 0, 27, 3, 2, 11, 5)
    out = torch.from_numpy(G.pattern(640)).cuda()
    ops.ragged_gather(arena, None, desc, out)
    want = G.pattern(640)
    want[:459] = img.reshape(-1)
    want[460:460 + 165] = img[3:14, 2:7].reshape(-1)
    assert np.array_equal(out.cpu().numpy(), want)
    del arena
    torch.cuda.empty_cache()


# ---- the loader --------------------------------------------------------------------------------------------------------------------
def _compare(ds, n_batches, cache_bytes, dev_ds=None, **kw):
    """The host pipeline beside the device pipeline with the cache on, n_batches batches: equal dicts, bitwise.  Returns the
    loader's stats, the stats after every batch and the images served."""
    dev_kw = {k: kw.pop(k) for k in ("jpeg_decode", "jpeg_entropy") if k in kw}
    host = load_batch_with_text(ds, pipeline='host', **kw)
    trail = []
    with load_batch_with_text(dev_ds or ds, pipeline='device', workers=4, cache='device', cache_bytes=cache_bytes, **dev_kw, **kw) as dev:
        for i in range(n_batches):
            a, b = next(host), next(dev)
            assert set(a) == set(b) == set(KEYS)
            for k in KEYS:
                assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, (i, k)
                assert torch.equal(a[k], b[k]), "batch %d key %s differs" % (i, k)
            trail.append(dev.cache_stats())
        stats = dev.cache_stats()
    host.close()
    return stats, trail, n_batches * kw["batch_size"]


@pytest.fixture
def reads(monkeypatch):
    """Every datasets.tfrecord.read_records call the DEVICE loader's threads make, as (path) in call order."""
    calls = []
    real = T.read_records

    def counted(path):
        if threading.current_thread().name == "ds-input-feeder":
            calls.append(path)
        return real(path)

    monkeypatch.setattr(T, "read_records", counted)
    return calls


ARMS = {"pil": {}, "jpeg": dict(jpeg_decode="device"), "entropy": dict(jpeg_decode="device", jpeg_entropy="device")}


@pytest.mark.parametrize("arm", sorted(ARMS))
@pytest.mark.parametrize("is_training", (False, True))
@pytest.mark.parametrize("shuffle", (True, False))
def test_same_batches_with_the_cache_on(tmp_path, reads, arm, is_training, shuffle):
    root = str(tmp_path / "d")
    ds = _jpeg_dataset(root)
    dev_ds = None
    if arm == "entropy":                           # the restart-marked copy: the same pixels, so the same host batches
        assert cd.add_restart_markers(root)[0] == 22 + 6
        dev_ds = cd.get_split_with_text("train", root, tfrecords_subdir="tfrecords_rst")
    n = 3 * 22 // 4 + 2                            # three passes and a bit
    stats, trail, served = _compare(ds, n, 64 * MB, dev_ds, batch_size=4, shuffle=shuffle, seed=5, height=224, width=224,
                                    is_training=is_training, max_token_id=100, num_classes=3, **ARMS[arm])
    assert stats["misses"] == 22 and stats["hits"] == served - 22 and stats["spilled"] == 0
    assert stats["records"] == 22 and 0 < stats["bytes_used"] <= stats["bytes_capacity"] == 64 * MB
    assert trail[5]["misses"] == 22 and trail[4]["hits"] == 0        # pass 0 is batches 0..5 (22 = 5 * 4 + 2)
    assert len(reads) == 2 and len(set(reads)) == 2                  # each shard once, in pass 0: nothing is read after it


@pytest.mark.parametrize("is_training", (False, True))
def test_an_arena_too_small_spills_and_keeps_the_batches(tmp_path, is_training):
    ds = _jpeg_dataset(str(tmp_path / "d"))
    full, _, _ = _compare(ds, 6, 64 * MB, batch_size=4, shuffle=True, seed=5, height=224, width=224, is_training=is_training)
    half = full["bytes_used"] // 2
    stats, trail, served = _compare(ds, 3 * 22 // 4 + 1, half, batch_size=4, shuffle=True, seed=5, height=224, width=224,
                                    is_training=is_training, jpeg_decode="device" if is_training else "host")
    assert stats["spilled"] > 0 and stats["bytes_used"] <= stats["bytes_capacity"] == half
    assert stats["hits"] + stats["misses"] == served and 0 < stats["records"] < 22
    first = next(i for i, t in enumerate(trail) if t["spilled"])
    assert all(t["records"] == trail[first]["records"] for t in trail[first:])      # nothing is inserted once it is full
    assert stats["hits"] > 0 and stats["spilled"] == stats["misses"] - stats["records"]


@pytest.mark.parametrize("rank", (0, 1))
def test_data_parallel_ranks_with_the_cache_on(tmp_path, rank):
    ds = _jpeg_dataset(str(tmp_path / "d"))
    stats, _, served = _compare(ds, 3 * 11 // 3, 64 * MB, batch_size=3, shuffle=True, seed=2, height=224, width=224, rank=rank,
                                world=2, jpeg_decode="device")
    assert stats["hits"] + stats["misses"] == served and stats["spilled"] == 0 and stats["records"] == stats["misses"] <= 22


def _odd_sizes_dataset(root):
    """Nine records in two shards: 1 x 1, 3 x 5, 500 x 375 and a few between, PNG and JPEG."""
    from PIL import Image
    os.makedirs(root)
    rng = np.random.RandomState(8)
    sizes = ((1, 1), (3, 5), (375, 500), (5, 3), (2, 40), (40, 2), (64, 48), (1, 9), (33, 17))
    paths = []
    for shard in range(2):
        recs = []
        for i in range(shard, len(sizes), 2):
            h, w = sizes[i]
            img = rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
            b = io.BytesIO()
            Image.fromarray(img).save(b, format="PNG" if i % 3 else "JPEG", quality=90)
            recs.append(du.image_to_tfexample_with_text(b.getvalue(), b'x', h, w, rng.randint(0, 100, 50).tolist(), 7, i % 3, 100 + i, i % 7))
        paths.append(os.path.join(root, "tumblr_train_%05d-of-00002.tfrecord" % shard))
        T.write_records(paths[-1], recs)
    return cd.Dataset(paths, len(sizes), 3, {0: "a", 1: "b", 2: "c"})


@pytest.mark.parametrize("is_training", (False, True))
def test_other_sizes_and_formats(tmp_path, is_training):
    ds = _odd_sizes_dataset(str(tmp_path / "odd"))
    for arm in ("pil", "jpeg"):
        stats, _, served = _compare(ds, 7, 8 * MB, batch_size=4, shuffle=True, seed=1, height=224, width=224, is_training=is_training,
                                    **ARMS[arm])
        assert stats["misses"] == 9 and stats["hits"] == served - 9
    png = _png_dataset(str(tmp_path / "png"))
    stats, _, served = _compare(png, 3 * 11 // 4 + 1, 8 * MB, batch_size=4, shuffle=True, seed=5, height=224, width=224,
                                is_training=is_training)
    assert stats["misses"] == 11 and stats["hits"] == served - 11


def _failing_batch(ds, **kw):
    it = load_batch_with_text(ds, batch_size=4, height=224, width=224, **kw)
    try:
        for i in range(50):
            try:
                next(it)
            except StopIteration:
                return None
            except Exception as e:
                return i, type(e)
    finally:
        it.close()


def test_a_corrupt_record_raises_at_the_same_batch_whenever_it_is_met(tmp_path):
    ds = _jpeg_dataset(str(tmp_path / "d"), corrupt=5)
    cache = dict(pipeline='device', workers=4, cache='device', cache_bytes=64 * MB)
    h = _failing_batch(ds, pipeline='host', shuffle=False)
    assert h is not None and h == _failing_batch(ds, shuffle=False, **cache) == _failing_batch(ds, shuffle=False, jpeg_decode="device", **cache)
    # two ranks, shuffled: rank r meets record 5 in the first pass in which it falls to it -- pass 0 for one of them, a
    # later pass (its neighbours resident by then) for the other; never cached, it raises there as on the host
    met = []
    for rank in (0, 1):
        kw = dict(shuffle=True, seed=2, rank=rank, world=2)
        h = _failing_batch(ds, pipeline='host', **kw)
        assert h is not None and h == _failing_batch(ds, **kw, **cache), rank
        met.append(h[0])
    assert min(met) <= 1 and max(met) >= 2           # 11 records of a rank per pass: batches 0 and 1 are pass 0's


def test_bad_tokens_labels_and_refused_switches(tmp_path):
    ds = _jpeg_dataset(str(tmp_path / "d"))
    for kw, exc in ((dict(max_token_id=50), "exceeds the embedding table"), (dict(num_classes=2), "outside")):
        for extra in (dict(pipeline="host"), dict(pipeline="device", cache="device", cache_bytes=64 * MB)):
            it = load_batch_with_text(ds, batch_size=4, shuffle=False, height=224, width=224, **extra, **kw)
            with pytest.raises(ValueError, match=exc):
                for _ in range(20):
                    next(it)
            it.close()
    with pytest.raises(ValueError, match="pipeline='device'"):
        load_batch_with_text(ds, pipeline='host', cache='device', cache_bytes=MB)
    with pytest.raises(ValueError, match="cache_bytes"):
        load_batch_with_text(ds, pipeline='device', cache='device')
    with pytest.raises(ValueError, match="CUDA/HIP device"):
        load_batch_with_text(ds, pipeline='device', device="cpu", cache='device', cache_bytes=MB)


def test_closing_mid_pass_joins_every_thread_and_frees_the_arena(tmp_path):
    ds = _jpeg_dataset(str(tmp_path / "d"))
    gc.collect()
    torch.cuda.synchronize()
    before, mem = threading.active_count(), torch.cuda.memory_allocated()
    it = load_batch_with_text(ds, batch_size=4, height=224, width=224, pipeline='device', workers=4, cache='device', cache_bytes=96 * MB)
    next(it), next(it)
    assert threading.active_count() >= before + 5 and len(it.threads()) == 5
    held = torch.cuda.memory_allocated()
    assert held >= mem + 96 * MB
    it.close()
    assert threading.active_count() == before and it.threads() == []
    assert next(it, None) is None
    gc.collect()
    assert torch.cuda.memory_allocated() <= held - 96 * MB


def test_a_trainer_runs_the_same_with_the_cache_on(tmp_path):
    from tumblr_emotions_amd.image_text_model.im_text_rnn_model import train_deep_sentiment
    root = str(tmp_path / "data")
    _jpeg_dataset(root)
    base = dict(_glove(root), input_pipeline='device', input_workers=4)
    out = {}
    for cache in ("none", "device"):
        torch.manual_seed(0)
        np.random.seed(0)
        train_dir = str(tmp_path / ("train_" + cache))
        cfg = dict(base, input_cache=cache, input_cache_gb=0.05) if cache == "device" else dict(base, input_cache=cache)
        loss = train_deep_sentiment(None, train_dir, 12, config=cfg, quiet=True)          # 12 steps of 4: past two passes of 22
        out[cache] = (loss, _checkpoint(train_dir))
    assert out["none"][0] == out["device"][0]
    a, b = out["none"][1], out["device"][1]
    assert sorted(a) == sorted(b) and len(a) > 10
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def _checkpoint(train_dir):
    from tumblr_emotions_amd.training import latest_checkpoint
    ck = torch.load(latest_checkpoint(train_dir), map_location="cpu", weights_only=True)
    assert ck["global_step"] == 12
    out = {k: v.numpy() for k, v in ck["variables"].items()}
    out.update(adam_m=ck["adam_m"].numpy(), adam_v=ck["adam_v"].numpy())
    return out
