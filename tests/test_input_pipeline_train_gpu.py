"""is_training=True end to end: pipeline='device' (ds_preprocess_train) yields the augmented batches of pipeline='host' bit
for bit, for any worker count and for the ranks of a data-parallel world; the trainers honour config['augment'], the
evaluators never do.  Datasets are generated in tmp_path from seeds; nothing is committed."""
import gc
import threading

import numpy as np
import pytest
import torch

from test_input_pipeline_gpu import KEYS, _glove, _jpeg_dataset, _same_stream
from tumblr_emotions_amd.image_model.im_model import load_batch_with_text
from tumblr_emotions_amd.input_pipeline import DeviceLoader

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("workers", (1, 8))
def test_device_pipeline_yields_the_host_pipelines_augmented_batches(tmp_path, workers):
    ds = _jpeg_dataset(str(tmp_path / "d"))
    n = ds.num_samples
    assert n % 4 != 0
    before = threading.active_count()
    # two passes and a bit with shuffling: the pass number and the global record index key the draws in both pipelines
    got = _same_stream(ds, 2 * n // 4 + 2, batch_size=4, shuffle=True, height=224, width=224, workers=workers, seed=5,
                       max_token_id=100, num_classes=3, is_training=True)
    assert got == 2 * n // 4 + 2
    assert _same_stream(ds, 100, batch_size=4, shuffle=False, height=299, width=299, workers=workers, seed=5, loop=False,
                        is_training=True) == n // 4
    assert threading.active_count() == before                   # _same_stream closed its loaders: no live thread


@pytest.mark.parametrize("rank", (0, 1))
def test_data_parallel_shards_are_augmented_alike_in_both_pipelines(tmp_path, rank):
    ds = _jpeg_dataset(str(tmp_path / "d"))
    # 22 records, 11 per rank: 9 batches of 3 run into the third pass
    assert _same_stream(ds, 9, batch_size=3, shuffle=True, height=224, width=224, rank=rank, world=2, seed=2, workers=8,
                        is_training=True) == 9


def test_augmented_batches_differ_from_eval_batches_in_the_images_only(tmp_path):
    ds = _jpeg_dataset(str(tmp_path / "d"))
    kw = dict(batch_size=4, shuffle=True, height=224, width=224, seed=3, pipeline='device', workers=8)
    with load_batch_with_text(ds, **kw) as plain, load_batch_with_text(ds, is_training=True, **kw) as aug:
        assert isinstance(aug, DeviceLoader)
        firsts = {}
        for i in range(2 * (ds.num_samples // 4) + 1):
            a, b = next(plain), next(aug)
            for k in KEYS[1:]:
                assert torch.equal(a[k], b[k]), (i, k)
            assert a["images"].shape == b["images"].shape and not torch.equal(a["images"], b["images"])
            assert float(b["images"].min()) >= -1.0 and float(b["images"].max()) <= 1.0
            for j, p in enumerate(b["post_ids"].tolist()):           # a record seen again (next pass) is augmented anew
                if p in firsts:
                    assert not torch.equal(firsts[p], b["images"][j])
                else:
                    firsts[p] = b["images"][j].clone()
    assert aug.threads() == [] and plain.threads() == []


def test_closing_an_augmenting_loader_joins_every_thread(tmp_path):
    ds = _jpeg_dataset(str(tmp_path / "d"))
    before = threading.active_count()
    it = load_batch_with_text(ds, batch_size=4, height=224, width=224, pipeline='device', workers=8, is_training=True)
    next(it), next(it)
    assert len(it.threads()) == 9
    it.close()
    assert threading.active_count() == before and it.threads() == []
    assert next(it, None) is None


def test_trainers_augment_and_evaluators_do_not(tmp_path, capsys):
    from tumblr_emotions_amd.image_model.im_model import ImageModel, evaluate_image_model, train_image_model
    from tumblr_emotions_amd.image_model.im_model import _CONFIG as IM_CONFIG
    from tumblr_emotions_amd.image_text_model.im_text_rnn_model import (DeepSentiment, evaluate_deep_sentiment,
                                                                       train_deep_sentiment)
    root = str(tmp_path / "data")
    _jpeg_dataset(root)
    plain = dict(_glove(root), input_pipeline='device', input_workers=4)
    cfg = dict(plain, augment=True)
    gc.collect()
    before = threading.active_count()

    def logged_losses():
        out = capsys.readouterr().out
        vals = [float(l.split("loss = ")[1].split()[0]) for l in out.splitlines() if l.startswith("global step")]
        assert vals and all(np.isfinite(v) for v in vals), out
        return vals

    train_dir = str(tmp_path / "train")
    assert np.isfinite(train_deep_sentiment(None, train_dir, 3, config=cfg))
    logged_losses()
    acc = evaluate_deep_sentiment(train_dir, str(tmp_path / "log"), "validation", 3, config=cfg, quiet=True)
    assert 0.0 <= acc <= 1.0
    im_dir = str(tmp_path / "train_im")
    im_cfg = dict(dataset_dir=root, batch_size=4, input_pipeline='device', input_workers=4, augment=True)
    assert np.isfinite(train_image_model(None, im_dir, 3, config=im_cfg))
    logged_losses()
    acc = evaluate_image_model(im_dir, str(tmp_path / "log_im"), "validation", 3, config=im_cfg, quiet=True)
    assert 0.0 <= acc <= 1.0

    # what the front ends read: a model built the way evaluate_* build theirs reads eval-chain batches whether or not the key
    # is set; the same model after use_augmentation() -- what the trainers call -- reads the augmented ones
    full = dict(mode="train", initial_lr=1e-3, decay_factor=0.3, im_features_size=256, fc_size=512, final_endpoint="Mixed_5c")
    models = [DeepSentiment(dict(full, **cfg)), DeepSentiment(dict(full, **plain)), DeepSentiment(dict(full, **cfg)),
              ImageModel(dict(IM_CONFIG, **im_cfg)), ImageModel(dict(IM_CONFIG, **dict(im_cfg, augment=False)))]
    models[2].use_augmentation()
    b = [m.next_batch(0) for m in models]
    assert all(isinstance(m._records, DeviceLoader) for m in models)
    for k in KEYS:
        assert torch.equal(b[0][k], b[1][k]), k
        assert torch.equal(b[3][k], b[4][k]), k
        assert torch.equal(b[0][k], b[2][k]) == (k != "images"), k
    host = next(load_batch_with_text(models[0].dataset, 4, height=224, width=224, is_training=True, max_token_id=10 ** 6))
    assert torch.equal(host["images"], b[2]["images"])               # ... and they are the host generator's augmented batch
    with pytest.raises(RuntimeError, match="first batch"):
        models[0].use_augmentation()
    with pytest.raises(ValueError, match="augment"):
        ImageModel(dict(IM_CONFIG, synthetic=True, augment=True))
    for m in models:
        m._records.close()
    del models, m, b
    gc.collect()
    assert threading.active_count() == before
