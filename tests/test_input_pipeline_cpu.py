"""Host logic of the device input pipeline, no GPU: the descriptor builder against central_crop / resize_bilinear's own
expressions, the ragged packer and its bounds check, the ordered pool, the worker clamp, thread lifetime."""
import os
import threading
import time

import numpy as np
import pytest
import torch

from tumblr_emotions_amd import input_pipeline as P
from tumblr_emotions_amd import ops
from tumblr_emotions_amd.preprocessing import inception_preprocessing as ip

SIZES = [(1, 1), (7, 3), (224, 224), (256, 256), (333, 499), (375, 500), (50, 1000), (1500, 2000)]


def test_crop_box_equals_central_crop_on_a_grid():
    """Offsets and extents for every (h, w) in 1..64 squared plus the kernel test's sizes: central_crop is run on an
    index image, so the slice it took can be read back from its corners."""
    grid = [(h, w) for h in range(1, 65) for w in range(1, 65)] + SIZES
    for h, w in grid:
        idx = np.arange(h * w, dtype=np.int64).reshape(h, w, 1)
        want = ip.central_crop(idx, 0.875)
        y0, x0, ch, cw = P.crop_box(h, w)
        assert want.shape[:2] == (ch, cw), (h, w)
        assert ch >= 1 and cw >= 1 and 0 <= y0 and y0 + ch <= h and 0 <= x0 and x0 + cw <= w
        assert np.array_equal(want, idx[y0:y0 + ch, x0:x0 + cw]), (h, w)
    assert P.crop_box(256, 256) == (16, 16, 224, 224)


def test_scales_equal_resize_bilinears_axis():
    """resize_bilinear samples at arange(n_out, f32) * f32(n_in / n_out): the scale is compared bitwise with that
    expression, and a ramp image resized along one axis reproduces src = o * scale wherever nothing is clamped."""
    ns = sorted({P.crop_box(h, 1)[2] for h in range(1, 65)} | {P.crop_box(h, w)[k] for h, w in SIZES for k in (2, 3)})
    for n_out in (224, 299):
        for n_in in ns:
            s = P.resize_scale(n_in, n_out)
            assert s.dtype == np.float32 and s.tobytes() == np.float32(n_in / n_out).tobytes()
            ramp = np.arange(n_in, dtype=np.float32).reshape(n_in, 1, 1)
            got = ip.resize_bilinear(ramp, n_out, 1)[:, 0, 0]
            src = np.arange(n_out, dtype=np.float32) * s
            lo = np.floor(src)
            inner = lo + 1 <= n_in - 1
            want = (lo + (src - lo).astype(np.float32)).astype(np.float32)       # ramp: a + (a + 1 - a) * f
            assert np.array_equal(got[inner], want[inner]), (n_in, n_out)


def test_pack_ragged_offsets_descriptors_and_bounds():
    rng = np.random.RandomState(0)
    shapes = [(1, 1), (5, 3), (37, 41), (2, 7)]
    images = [rng.randint(0, 256, size=(h, w, 3)).astype(np.uint8) for h, w in shapes]
    buf, desc, used = P.pack_ragged(images, 224, 299)
    assert desc.dtype == ops.preprocess_desc_dtype() and desc.dtype.itemsize == 24 and len(desc) == 4
    pos = 0
    for im, d in zip(images, desc):
        assert d["offset"] == pos and d["offset"] % 4 == 0 and (d["height"], d["width"]) == im.shape[:2]
        assert np.array_equal(buf[pos:pos + im.size].reshape(im.shape), im)
        assert d["scale_y"] == np.float32(im.shape[0] / 224) and d["scale_x"] == np.float32(im.shape[1] / 299)
        pos = -(-(pos + im.size) // 4) * 4
    assert used == pos and buf.size >= used
    ops.check_preprocess_descs(desc, used)                       # fits
    # a destination that is too small is refused by the packer
    with pytest.raises(ValueError, match="do not fit"):
        P.pack_ragged(images, 224, 224, out=np.zeros(used - 1, np.uint8))
    # a descriptor past the buffer is rejected before any launch (no device is needed to be refused)
    with pytest.raises(ValueError, match="does not fit"):
        ops.check_preprocess_descs(desc, used - 8)
    for field, value in (("offset", -4), ("height", 0), ("width", -1), ("height", 38)):
        bad = desc.copy()
        bad[field][2] = value
        with pytest.raises(ValueError, match="does not fit"):
            ops.check_preprocess_descs(bad, used)
    bad = desc.copy()
    bad["offset"][3] = used
    with pytest.raises(ValueError, match="descriptor 3"):
        ops.check_preprocess_descs(bad, used)
    bad = desc.copy()
    bad["scale_x"][0] = np.nan
    with pytest.raises(ValueError, match="scales"):
        ops.check_preprocess_descs(bad, used)
    with pytest.raises(ValueError):
        ops.check_preprocess_descs(np.zeros(3, np.int64), 100)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.preprocess_eval(torch.from_numpy(buf), desc, 224, 224)


def test_pool_returns_results_in_submission_order_when_early_items_are_slow():
    pool = P.OrderedPool(4)
    try:
        done = []

        def work(i):
            time.sleep(0.15 if i < 2 else 0.0)
            done.append(i)
            return i * i

        slots = [pool.submit(work, i) for i in range(12)]
        assert [s.result() for s in slots] == [i * i for i in range(12)]
        assert sorted(done) == list(range(12)) and done[:2] != [0, 1]       # later items really finished first

        def boom():
            raise KeyError("x")

        ok, bad, ok2 = pool.submit(work, 3), pool.submit(boom), pool.submit(work, 4)
        assert ok.result() == 9
        with pytest.raises(KeyError):
            bad.result()                                          # raised where it is consumed, not in the worker
        assert ok2.result() == 16
    finally:
        pool.close()


def test_workers_are_clamped_to_16():
    before = threading.active_count()
    assert P.clamp_workers(40) == 16 and P.clamp_workers(0) == 1 and P.clamp_workers(8) == 8
    pool = P.OrderedPool(40)
    assert pool.workers == 16 and threading.active_count() == before + 16
    pool.close()
    assert threading.active_count() == before


def _text_dataset(root):
    from test_datasets_cpu import _make_dataset
    from tumblr_emotions_amd.datasets import convert_to_dataset as cd
    os.makedirs(root)
    _make_dataset(root, n_train=23, n_valid=3)
    return cd.get_split_with_text("train", root)


def test_closing_a_half_consumed_loader_joins_its_threads(tmp_path):
    from tumblr_emotions_amd.image_model.im_model import load_batch_with_text
    ds = _text_dataset(str(tmp_path / "d"))
    before = threading.active_count()
    it = load_batch_with_text(ds, batch_size=4, device="cpu", pipeline='device', workers=40, decode_images=False)
    assert it.workers == 16
    next(it), next(it)
    assert threading.active_count() == before + 17                # feeder + 16 decode workers
    it.close()
    assert threading.active_count() == before and it.threads() == []
    with pytest.raises(StopIteration):
        next(it)
    with load_batch_with_text(ds, batch_size=4, device="cpu", pipeline='device', workers=3, decode_images=False) as it:
        next(it)
    assert threading.active_count() == before


def test_text_only_batches_match_the_host_pipeline_without_a_device(tmp_path):
    """decode_images=False needs no kernel, so the ordering logic (source shuffle, batch permutation, ragged tail, ranks,
    loop=False) can be compared on the CPU; the GPU suite repeats it with images."""
    from tumblr_emotions_amd.image_model.im_model import load_batch_with_text
    ds = _text_dataset(str(tmp_path / "d"))
    for shuffle in (True, False):
        for loop in (True, False):
            for world, rank in ((1, 0), (2, 0), (2, 1)):
                kw = dict(batch_size=4, shuffle=shuffle, device="cpu", rank=rank, world=world, loop=loop, seed=3,
                          decode_images=False, max_token_id=100, num_classes=3)
                host = load_batch_with_text(ds, pipeline='host', **kw)
                with load_batch_with_text(ds, pipeline='device', workers=4, **kw) as dev:
                    n = 0
                    for _ in range(14):
                        a, b = next(host, None), next(dev, None)
                        if a is None or b is None:
                            assert a is None and b is None
                            break
                        assert set(a) == set(b) == {"texts", "seq_lens", "labels", "post_ids", "days"}
                        assert all(torch.equal(a[k], b[k]) and a[k].dtype == b[k].dtype for k in a)
                        n += 1
                    assert n == (14 if loop else (23 // world + (rank < 23 % world)) // 4)


def test_images_on_a_cpu_device_are_an_error_not_a_fallback(tmp_path):
    from tumblr_emotions_amd.image_model.im_model import load_batch_with_text
    ds = _text_dataset(str(tmp_path / "d"))
    with load_batch_with_text(ds, batch_size=4, device="cpu", pipeline='device', workers=2) as it:
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            next(it)
    with pytest.raises(ValueError):
        load_batch_with_text(ds, pipeline='elsewhere')
