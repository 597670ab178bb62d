"""pipeline='device' yields the batches of pipeline='host': every key, bitwise, in the same order -- and the front ends
run on it.  Datasets are generated in tmp_path from seeds; nothing is committed."""
import gc
import io
import os
import threading

import numpy as np
import pytest
import torch

from tumblr_emotions_amd.datasets import convert_to_dataset as cd
from tumblr_emotions_amd.datasets import dataset_utils as du
from tumblr_emotions_amd.datasets import tfrecord as T
from tumblr_emotions_amd.image_model.im_model import load_batch_with_text
from tumblr_emotions_amd.input_pipeline import DeviceLoader

pytestmark = pytest.mark.gpu
KEYS = ("images", "texts", "seq_lens", "labels", "post_ids", "days")


def _jpeg_dataset(root, n_train=22, n_valid=6, corrupt=None, garbage_images=False, seed=11):
    """Mixed-size JPEGs (smooth content + noise) in two shards per split, written with the package's own writer.
    corrupt: index of a train record whose JPEG payload is cut short; garbage_images: every payload is random bytes."""
    from PIL import Image
    os.makedirs(os.path.join(root, "photos"))
    os.makedirs(os.path.join(root, "tfrecords"))
    du.write_label_file({0: "happy", 1: "sad", 2: "angry"}, root, "photos")
    with open(os.path.join(root, "photos", cd._TRAIN_VALID_FILENAME), "w") as f:
        f.write("train:%d\nvalidation:%d\n" % (n_train, n_valid))
    rng = np.random.RandomState(seed)
    for split, n in (("train", n_train), ("validation", n_valid)):
        recs = [[], []]
        for i in range(n):
            h, w = int(rng.randint(20, 400)), int(rng.randint(20, 520))
            yy, xx = np.mgrid[0:h, 0:w]
            base = np.stack([128 + 100 * np.sin(yy / 17.0 + i), 128 + 100 * np.cos(xx / 23.0), (yy + xx) % 256], axis=2)
            img = np.clip(base + rng.normal(0, 8, size=(h, w, 3)), 0, 255).astype(np.uint8)
            b = io.BytesIO()
            Image.fromarray(img).save(b, format="JPEG", quality=90)
            data = b.getvalue()
            if garbage_images:
                data = rng.bytes(200)
            elif split == "train" and i == corrupt:
                data = data[:len(data) // 3]
            text = rng.randint(0, 100, size=50).tolist()
            recs[i % 2].append(du.image_to_tfexample_with_text(data, b'jpg', h, w, text, 5 + i % 40, i % 3, 2000 + i, i % 7))
        for shard in range(2):
            T.write_records(cd.dataset_filename(root, "tfrecords", split, shard, 2), recs[shard])
    return cd.get_split_with_text("train", root)


def _png_dataset(root):
    from test_datasets_cpu import _make_dataset
    os.makedirs(root)
    _make_dataset(root, n_train=11, n_valid=3)
    return cd.get_split_with_text("train", root)


def _same_stream(ds, n_batches, **kw):
    """Both pipelines side by side for n_batches (or to the end of the data): equal dicts, bitwise; returns the count."""
    workers = kw.pop("workers", 4)
    prefetch = kw.pop("prefetch", 2)
    host = load_batch_with_text(ds, pipeline='host', **kw)
    dev = load_batch_with_text(ds, pipeline='device', workers=workers, prefetch=prefetch, **kw)
    assert isinstance(dev, DeviceLoader)
    try:
        count = 0
        for i in range(n_batches):
            a, b = next(host, None), next(dev, None)
            if a is None or b is None:
                assert a is None and b is None, "the pipelines end at different batches (%d)" % i
                break
            assert set(a) == set(b) == set(KEYS)
            for k in KEYS:
                assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].device == b[k].device, (i, k)
                assert torch.equal(a[k], b[k]), "batch %d key %s differs" % (i, k)
            count += 1
        return count
    finally:
        dev.close()


@pytest.mark.parametrize("kind", ("png", "jpeg"))
@pytest.mark.parametrize("shuffle", (True, False))
@pytest.mark.parametrize("workers", (1, 4))
def test_device_pipeline_yields_the_host_pipelines_batches(tmp_path, kind, shuffle, workers):
    ds = _png_dataset(str(tmp_path / "d")) if kind == "png" else _jpeg_dataset(str(tmp_path / "d"))
    n = ds.num_samples
    # two epochs and a bit, batch 4: the ragged tail of an epoch is carried into the next one
    assert n % 4 != 0
    got = _same_stream(ds, 2 * n // 4 + 2, batch_size=4, shuffle=shuffle, height=224, width=224, workers=workers, seed=5,
                       max_token_id=100, num_classes=3)
    assert got == 2 * n // 4 + 2
    # loop=False: both end at the same batch
    assert _same_stream(ds, 100, batch_size=4, shuffle=shuffle, height=224, width=224, workers=workers, seed=5, loop=False) == n // 4


@pytest.mark.parametrize("rank", (0, 1))
def test_data_parallel_shards(tmp_path, rank):
    ds = _jpeg_dataset(str(tmp_path / "d"))
    assert _same_stream(ds, 9, batch_size=3, shuffle=True, height=224, width=224, rank=rank, world=2, seed=2) == 9
    assert _same_stream(ds, 100, batch_size=3, shuffle=False, height=299, width=299, rank=rank, world=2, loop=False) == 11 // 3


def test_default_output_size_and_prefetch_depths(tmp_path):
    ds = _jpeg_dataset(str(tmp_path / "d"))
    for prefetch in (1, 2, 4):
        assert _same_stream(ds, 7, batch_size=5, shuffle=True, seed=9, prefetch=prefetch) == 7       # 299 x 299, the default


def test_corrupt_jpeg_raises_at_the_same_batch(tmp_path):
    ds = _jpeg_dataset(str(tmp_path / "d"), corrupt=10)

    def failing_batch(**kw):
        it = load_batch_with_text(ds, batch_size=4, shuffle=False, height=224, width=224, **kw)
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

    h = failing_batch(pipeline='host')
    d = failing_batch(pipeline='device', workers=4)
    assert h is not None and h == d, (h, d)


def test_bad_token_and_label_raise_in_both(tmp_path):
    ds = _jpeg_dataset(str(tmp_path / "d"))
    for kw, exc in ((dict(max_token_id=50), "exceeds the embedding table"), (dict(num_classes=2), "outside")):
        for pipeline in ("host", "device"):
            it = load_batch_with_text(ds, batch_size=4, shuffle=False, height=224, width=224, pipeline=pipeline, **kw)
            with pytest.raises(ValueError, match=exc):
                for _ in range(20):
                    next(it)
            it.close()


def test_closing_mid_epoch_joins_every_thread(tmp_path):
    ds = _jpeg_dataset(str(tmp_path / "d"))
    before = threading.active_count()
    it = load_batch_with_text(ds, batch_size=4, height=224, width=224, pipeline='device', workers=4)
    next(it), next(it)
    assert threading.active_count() >= before + 5 and len(it.threads()) == 5
    it.close()
    assert threading.active_count() == before and it.threads() == []
    assert next(it, None) is None
    it = load_batch_with_text(ds, batch_size=4, height=224, width=224, pipeline='device', workers=2)
    next(it)
    del it                                               # garbage collection stops the workers too
    gc.collect()
    assert threading.active_count() == before


def _glove(root):
    rng = np.random.RandomState(3)
    os.makedirs(os.path.join(root, "text_model", "embedding_weights"))
    with open(os.path.join(root, "text_model", "embedding_weights", "glove.test.20d.txt"), "w") as f:
        for i, row in enumerate(rng.normal(0, 0.4, size=(100, 20)).astype(np.float32)):
            f.write("w%d %s\n" % (i, " ".join(repr(float(v)) for v in row)))
    return dict(dataset_dir=root, text_dir=os.path.join(root, "text_model"), emb_dir="embedding_weights",
                filename="glove.test.20d.txt", batch_size=4, rnn_size=32, post_size=50)


def test_front_ends_train_and_evaluate_on_the_device_pipeline(tmp_path):
    from tumblr_emotions_amd.image_text_model.im_text_rnn_model import (DeepSentiment, evaluate_deep_sentiment,
                                                                       train_deep_sentiment)
    root = str(tmp_path / "data")
    _jpeg_dataset(root)
    cfg = dict(_glove(root), input_pipeline='device', input_workers=4)
    gc.collect()
    before = threading.active_count()
    train_dir = str(tmp_path / "train")
    loss = train_deep_sentiment(None, train_dir, 3, config=cfg, quiet=True)
    assert np.isfinite(loss)
    acc = evaluate_deep_sentiment(train_dir, str(tmp_path / "log"), "validation", 3, config=cfg, quiet=True)
    assert 0.0 <= acc <= 1.0
    full = dict(mode="train", initial_lr=1e-3, decay_factor=0.3, im_features_size=256, fc_size=512, final_endpoint="Mixed_5c")
    m = DeepSentiment(dict(full, **cfg))
    b = m.next_batch(0)
    assert isinstance(m._records, DeviceLoader) and m._records.workers == 4
    h = DeepSentiment(dict(full, **dict(cfg, input_pipeline='host')))
    hb = h.next_batch(0)
    assert not isinstance(h._records, DeviceLoader)
    for k in KEYS:
        assert torch.equal(b[k], hb[k]), k
    m._records.close()
    del m, h
    gc.collect()
    assert threading.active_count() == before            # the trainers' loaders are gone with their models


@pytest.mark.parametrize("pipeline", ("host", "device"))
def test_text_model_never_decodes_an_image(tmp_path, pipeline):
    """Every image payload is random bytes: a text-only model must train (decode_images=False reaches both pipelines)."""
    from tumblr_emotions_amd.text_model.text_embedding import TextModel, _CONFIG, train_text_model
    root = str(tmp_path / "data")
    ds = _jpeg_dataset(root, garbage_images=True)
    with pytest.raises(Exception):                        # the payloads really are undecodable
        next(load_batch_with_text(ds, batch_size=4, height=224, width=224))
    cfg = dict(_glove(root), input_pipeline=pipeline)
    loss = train_text_model(str(tmp_path / "train"), 3, config=cfg, quiet=True)
    assert np.isfinite(loss)
    m = TextModel(dict(_CONFIG, **cfg))
    b = m.next_batch(0)
    assert "images" not in b and b["texts"].shape == (4, 50)
    assert isinstance(m._records, DeviceLoader) == (pipeline == "device")
    if pipeline == "device":
        m._records.close()
