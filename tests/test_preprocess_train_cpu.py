"""The train-time augmentation on the host, no GPU: the NumPy definition of preprocess_for_train (colour known answers,
flip, geometry), the crop sampler's distribution, the per-record random stream, the host generator with is_training=True,
the refused arguments and the layout of ds_preprocess_train_desc."""
import io
import math
import os
import re

import numpy as np
import pytest
import torch

from tumblr_emotions_amd import _lib, ops
from tumblr_emotions_amd import input_pipeline as P
from tumblr_emotions_amd.preprocessing import inception_preprocessing as ip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def _px(*rgb):
    return np.array(rgb, F).reshape(1, 1, 3)


def _params(h, w, flip=False, saturation_first=False, delta=0.0, factor=1.0, box=None):
    y0, x0, ch, cw = box or (0, 0, h, w)
    return ip.TrainParams(y0, x0, ch, cw, flip, saturation_first, F(delta), F(factor))


# ---- colour known answers (derived by hand from the fused AdjustSaturation formulas; exact) ---------------------------------
def test_saturation_known_answers():
    sat = lambda rgb, f: ip.adjust_saturation(_px(*rgb), F(f)).reshape(3).tolist()
    # factor 0: s = 0 -> c = 0, m = v: every channel becomes max(r, g, b)
    assert sat((0.2, 0.7, 0.4), 0) == [F(0.7)] * 3
    # pure red, factor 0.5: v = 1, s = 0.5, h = 0 -> c = 0.5, m = 0.5, f = 0 -> x = 0 -> (c + m, m, m)
    assert sat((1, 0, 0), 0.5) == [1.0, 0.5, 0.5]
    # factor 1.5 on pure red: s = min(1, 1.5) = 1 -> unchanged
    assert sat((1, 0, 0), 1.5) == [1.0, 0.0, 0.0]
    # grey: range = 0 -> s = 0, h = 0 -> (v, v, v) for any factor
    for f in (0, 0.5, 1, 1.4999, 7):
        for v in (0.0, 0.3, 1.0):
            assert sat((v, v, v), f) == [F(v)] * 3
    # factor 1 is not the identity in fp32
    assert sat((0.2, 0.7, 0.4), 1) == [F(0.19999999), F(0.7), F(0.40000004)]
    out = ip.adjust_saturation(np.random.RandomState(0).rand(5, 7, 3).astype(F), F(1.2))
    assert out.dtype == np.float32 and out.shape == (5, 7, 3)


def test_brightness_clip_and_scaling_known_answers():
    white, black = np.full((3, 4, 3), 255, np.uint8), np.zeros((3, 4, 3), np.uint8)
    for sat_first in (False, True):
        for factor in (0.5, 1.0, 1.5):
            up = ip.preprocess_for_train(white, 3, 4, _params(3, 4, delta=32 / 255, factor=factor, saturation_first=sat_first))
            dn = ip.preprocess_for_train(black, 3, 4, _params(3, 4, delta=-32 / 255, factor=factor, saturation_first=sat_first))
            assert up.dtype == np.float32 and (up == F(1.0)).all() and (dn == F(-1.0)).all()


def test_the_two_orderings_differ_where_they_must():
    """Pure red, delta d = +32/255, factor 1.5.  Brightness first: (1 + d, d, d) has v = 1 + d, range = 1, s = 1 / (1 + d)
    = 0.89, scaled by 1.5 and clamped to 1 -> c = v, m = 0, h = 0 -> (v, 0, 0), clipped to (1, 0, 0).  Saturation first:
    red stays (1, 0, 0) (s clamps at 1), then + d and the clip: (1, d, d)."""
    d = F(32 / 255)
    a = ip.distort_color_fast(_px(1, 0, 0), False, d, F(1.5)).reshape(3).tolist()
    b = ip.distort_color_fast(_px(1, 0, 0), True, d, F(1.5)).reshape(3).tolist()
    assert a == [1.0, 0.0, 0.0] and b == [1.0, d, d]
    red = np.zeros((2, 2, 3), np.uint8)
    red[..., 0] = 255
    a = ip.preprocess_for_train(red, 2, 2, _params(2, 2, delta=d, factor=1.5, saturation_first=False))
    b = ip.preprocess_for_train(red, 2, 2, _params(2, 2, delta=d, factor=1.5, saturation_first=True))
    assert (a == np.array([1, -1, -1], F)).all() and (b == np.array([1, (d - F(0.5)) * F(2), (d - F(0.5)) * F(2)], F)).all()


def test_flip_reverses_the_resized_image():
    im = np.random.RandomState(2).randint(0, 256, size=(37, 53, 3)).astype(np.uint8)
    for box in (None, (3, 5, 20, 31)):
        for sat_first in (False, True):
            kw = dict(delta=0.07, factor=1.3, saturation_first=sat_first, box=box)
            a = ip.preprocess_for_train(im, 24, 29, _params(37, 53, flip=False, **kw))
            b = ip.preprocess_for_train(im, 24, 29, _params(37, 53, flip=True, **kw))
            assert a.shape == (24, 29, 3) and np.array_equal(b, a[:, ::-1])
    assert not np.array_equal(a, b)


def test_geometry_equals_the_eval_chain_on_grey_images():
    """Crop = the whole image, no flip, delta 0: on a grey image the colour chain is exact for any factor, so what is left
    is convert + resize + scaling = preprocess_for_eval without the central crop."""
    rng = np.random.RandomState(3)
    for h, w in ((1, 1), (7, 3), (60, 31), (333, 499)):
        grey = np.repeat(rng.randint(0, 256, size=(h, w, 1)), 3, axis=2).astype(np.uint8)
        for out in (224, 299):
            for factor in (0.5, 1.0, 1.4999):
                got = ip.preprocess_for_train(grey, out, out, _params(h, w, factor=factor))
                assert np.array_equal(got, ip.preprocess_for_eval(grey, out, out, central_fraction=None))
    # and a crop is the eval chain of the slice
    got = ip.preprocess_for_train(grey, 224, 224, _params(333, 499, box=(10, 20, 100, 200)))
    assert np.array_equal(got, ip.preprocess_for_eval(grey[10:110, 20:220], 224, 224, central_fraction=None))


# ---- crop sampler -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(375, 500), (500, 375), (224, 224), (333, 499), (1200, 400)], ids=lambda s: "%dx%d" % s)
def test_crop_sampler_properties(size):
    H, W = size
    n = 10000
    heights = []
    for i in range(n):
        (y0, x0, ch, cw), attempts = ip._sample_crop(H, W, ip.record_rng(7, 0, i))
        assert attempts <= ip.MAX_ATTEMPTS, "draw %d fell back to the whole image" % i
        assert (y0, x0, ch, cw) == ip.sample_distorted_crop(H, W, ip.record_rng(7, 0, i))
        assert 0 <= y0 and 0 <= x0 and ch >= 1 and cw >= 1 and y0 + ch <= H and x0 + cw <= W
        assert 0.1 * W * H <= cw * ch <= 1.0 * W * H
        # crop_w == lrint(crop_h * a) for some a in [0.75, 1.33): the interval of such a is [(cw - .5) / ch, (cw + .5) / ch]
        assert (cw - 0.5) / ch <= 1.33 and (cw + 0.5) / ch >= 0.75, (ch, cw)
        heights.append(ch)
    # allowed heights: from the smallest crop of 10 % area at the widest aspect to the largest that fits
    lo = math.sqrt(0.1 * W * H / 1.33)
    hi = min(H, W / 0.75)
    q = np.histogram(heights, bins=4, range=(lo, hi))[0]
    assert (q > 0).all(), q
    assert min(heights) >= math.floor(lo) and max(heights) <= H


@pytest.mark.parametrize("size", [(50, 1000), (1000, 50)], ids=lambda s: "%dx%d" % s)
def test_crop_sampler_falls_back_to_the_whole_image_after_100_attempts(size):
    H, W = size
    for i in range(10000):
        box, attempts = ip._sample_crop(H, W, ip.record_rng(1, 2, i))
        assert box == (0, 0, H, W) and attempts == ip.MAX_ATTEMPTS + 1
    # every single attempt is rejected for these sizes
    u = np.random.RandomState(0).rand(2000, 4)
    assert all(ip._crop_attempt(H, W, *row) is None for row in u.tolist())


def test_one_pixel_image_is_accepted_at_the_first_attempt():
    for i in range(200):
        assert ip._sample_crop(1, 1, ip.record_rng(0, 0, i)) == ((0, 0, 1, 1), 1)


def test_train_params_ranges_and_draw_order():
    flips = firsts = 0
    n = 4000
    for i in range(n):
        p = ip.sample_train_params(375, 500, ip.record_rng(3, 1, i))
        assert isinstance(p.delta, np.float32) and isinstance(p.factor, np.float32)
        assert -32 / 255 - 1e-7 <= p.delta <= 32 / 255 + 1e-7 and 0.5 <= p.factor <= 1.5
        flips += p.flip
        firsts += p.saturation_first
        # the documented order: crop attempts first, then ONE call of four uniforms
        rng = ip.record_rng(3, 1, i)
        box = ip.sample_distorted_crop(375, 500, rng)
        u = rng.random(4)
        assert box == p[:4] and p.flip == (u[0] < 0.5) and p.saturation_first == (int(u[1] * 4) != 0)
        assert p.delta == F(-32 / 255 + u[2] * (64 / 255)) and p.factor == F(0.5 + u[3])
    assert abs(flips / n - 0.5) < 0.05 and abs(firsts / n - 0.75) < 0.05


# ---- random stream ----------------------------------------------------------------------------------------------------------
def test_record_stream_depends_on_seed_pass_and_index_only():
    draw = lambda *key: ip.sample_train_params(375, 500, ip.record_rng(*key))
    assert draw(5, 1, 17) == draw(5, 1, 17)
    assert draw(5, 1, 17) != draw(6, 1, 17) and draw(5, 1, 17) != draw(5, 2, 17) and draw(5, 1, 17) != draw(5, 1, 18)
    a, b = ip.record_rng(5, 1, 17).random(8), ip.record_rng(5, 1, 18).random(8)
    assert not np.intersect1d(a, b).size


def _jpeg_dataset(root, n_train=11, n_valid=3, seed=11):
    from PIL import Image
    from tumblr_emotions_amd.datasets import convert_to_dataset as cd
    from tumblr_emotions_amd.datasets import dataset_utils as du
    from tumblr_emotions_amd.datasets import tfrecord as T
    os.makedirs(os.path.join(root, "photos"))
    os.makedirs(os.path.join(root, "tfrecords"))
    du.write_label_file({0: "happy", 1: "sad", 2: "angry"}, root, "photos")
    with open(os.path.join(root, "photos", cd._TRAIN_VALID_FILENAME), "w") as f:
        f.write("train:%d\nvalidation:%d\n" % (n_train, n_valid))
    rng = np.random.RandomState(seed)
    for split, n in (("train", n_train), ("validation", n_valid)):
        recs = [[], []]
        for i in range(n):
            h, w = int(rng.randint(20, 120)), int(rng.randint(20, 160))
            yy, xx = np.mgrid[0:h, 0:w]
            base = np.stack([128 + 100 * np.sin(yy / 17.0 + i), 128 + 100 * np.cos(xx / 23.0), (yy + xx) % 256], axis=2)
            img = np.clip(base + rng.normal(0, 8, size=(h, w, 3)), 0, 255).astype(np.uint8)
            b = io.BytesIO()
            Image.fromarray(img).save(b, format="JPEG", quality=90)
            text = rng.randint(0, 100, size=50).tolist()
            recs[i % 2].append(du.image_to_tfexample_with_text(b.getvalue(), b'jpg', h, w, text, 5 + i % 40, i % 3, 2000 + i, i % 7))
        for shard in range(2):
            T.write_records(cd.dataset_filename(root, "tfrecords", split, shard, 2), recs[shard])
    return cd.get_split_with_text("train", root)


def test_host_generator_with_augmentation(tmp_path):
    from tumblr_emotions_amd.image_model.im_model import load_batch_with_text
    ds = _jpeg_dataset(str(tmp_path / "d"))
    kw = dict(batch_size=11, shuffle=True, height=32, width=32, device="cpu", seed=4, max_token_id=100, num_classes=3)
    plain = load_batch_with_text(ds, is_training=False, **kw)
    aug = load_batch_with_text(ds, is_training=True, **kw)
    again = load_batch_with_text(ds, is_training=True, **kw)
    passes = []
    for _ in range(2):                                   # batch = the whole pass
        a, b, c = next(plain), next(aug), next(again)
        for k in ("texts", "seq_lens", "labels", "post_ids", "days"):
            assert torch.equal(a[k], b[k]), k
        assert b["images"].shape == (11, 32, 32, 3) and b["images"].dtype == torch.float32
        assert float(b["images"].min()) >= -1.0 and float(b["images"].max()) <= 1.0
        assert not any(torch.equal(a["images"][j], b["images"][j]) for j in range(11))
        assert all(torch.equal(b[k], c[k]) for k in b)          # one seed: bit-identical runs
        passes.append(b)
    # the same record in pass 2 is augmented differently
    first = {int(p): passes[0]["images"][j] for j, p in enumerate(passes[0]["post_ids"])}
    for j, p in enumerate(passes[1]["post_ids"]):
        assert not torch.equal(first[int(p)], passes[1]["images"][j])
    other = next(load_batch_with_text(ds, is_training=True, **dict(kw, seed=5)))
    assert not torch.equal(other["images"], passes[0]["images"])


def test_data_parallel_ranks_use_the_global_record_index(tmp_path):
    """World 2: rank r's j-th record is global record 2 j + r of the pass, and its image is the one the world-1 stream
    gives that record."""
    from tumblr_emotions_amd.image_model.im_model import load_batch_with_text
    ds = _jpeg_dataset(str(tmp_path / "d"), n_train=12)
    kw = dict(shuffle=False, height=24, width=24, device="cpu", seed=9, is_training=True)
    whole = next(load_batch_with_text(ds, batch_size=12, **kw))
    for rank in (0, 1):
        part = next(load_batch_with_text(ds, batch_size=6, rank=rank, world=2, **kw))
        assert torch.equal(part["post_ids"], whole["post_ids"][rank::2])
        assert torch.equal(part["images"], whole["images"][rank::2])


# ---- refused arguments ------------------------------------------------------------------------------------------------------
def test_unimplemented_arguments_say_so():
    im = np.zeros((8, 8, 3), np.uint8)
    with pytest.raises(NotImplementedError, match="fast_mode"):
        ip.preprocess_image(im, 4, 4, is_training=True, fast_mode=False)
    with pytest.raises(NotImplementedError, match="bounding box"):
        ip.preprocess_image(im, 4, 4, is_training=True, bbox=np.array([[[0, 0, 1, 1]]], F))
    out = ip.preprocess_image(im, 4, 4, is_training=True, rng=ip.record_rng(0, 0, 0))
    assert out.shape == (4, 4, 3) and out.dtype == np.float32
    assert np.array_equal(ip.preprocess_image(im, 4, 4), ip.preprocess_for_eval(im, 4, 4))


def test_augment_with_synthetic_batches_is_an_error():
    from tumblr_emotions_amd.training import SyntheticInput

    class M(SyntheticInput):
        pass

    with pytest.raises(ValueError, match="augment"):
        M()._init_input({"synthetic": True, "augment": True}, 50, 100, 15, True, "cpu")
    m = M()
    m._init_input({"synthetic": True}, 50, 100, 15, True, "cpu")
    assert m._augment is False


# ---- descriptor layout ------------------------------------------------------------------------------------------------------
def test_train_descriptor_layout_matches_the_c_struct():
    import ctypes
    dt = ops.preprocess_train_desc_dtype()
    st = _lib.PreprocessTrainDesc
    assert dt.itemsize == ctypes.sizeof(st) == 40
    for name, _ in st._fields_:
        assert dt.fields[name][1] == getattr(st, name).offset, name
    # the .hip file asserts the same numbers on the C struct
    src = open(os.path.join(ROOT, "tumblr_emotions_amd", "csrc", "preprocess.hip")).read()
    m = re.search(r"static_assert\(sizeof\(ds_preprocess_train_desc\) == (\d+)(.*?);", src, flags=re.S)
    assert m and int(m.group(1)) == dt.itemsize
    offs = dict((k, int(v)) for k, v in re.findall(r"offsetof\(ds_preprocess_train_desc, (\w+)\) == (\d+)", m.group(2)))
    assert offs == {name: dt.fields[name][1] for name in dt.names}
    assert ops.preprocess_desc_dtype().itemsize == 24                     # the eval record is untouched


def test_pack_ragged_fills_train_descriptors_and_bad_ones_are_refused():
    rng = np.random.RandomState(0)
    crops = [rng.randint(0, 256, size=(h, w, 3)).astype(np.uint8) for h, w in ((5, 3), (37, 41), (2, 7))]
    params = [ip.TrainParams(1, 2, c.shape[0], c.shape[1], i == 1, i != 2, F(0.01 * i), F(0.5 + 0.3 * i)) for i, c in enumerate(crops)]
    buf, desc, used = P.pack_ragged(crops, 224, 299, params=params)
    assert desc.dtype == ops.preprocess_train_desc_dtype() and len(desc) == 3
    plain = P.pack_ragged(crops, 224, 299)[1]
    for k in ("offset", "height", "width", "scale_y", "scale_x"):
        assert np.array_equal(desc[k], plain[k])
    assert desc["flags"].tolist() == [2, 3, 0] and not desc["reserved"].any()
    assert desc["delta"].tolist() == [p.delta for p in params] and desc["factor"].tolist() == [p.factor for p in params]
    ops.check_preprocess_train_descs(desc, used)
    for field, value, msg in (("delta", np.nan, "finite"), ("factor", np.inf, "finite"), ("factor", -0.5, "factor"),
                              ("flags", 4, "flag"), ("reserved", 1, "flag"), ("height", 38, "does not fit"),
                              ("scale_x", 0, "scales")):
        bad = desc.copy()
        bad[field][1] = value
        with pytest.raises(ValueError, match=msg):
            ops.check_preprocess_train_descs(bad, used)
    with pytest.raises(ValueError):
        ops.check_preprocess_train_descs(plain, used)                     # the eval record is not a train record
    with pytest.raises(ValueError, match="not the crop"):
        P.pack_ragged(crops, 224, 224, params=params[::-1])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.preprocess_train(torch.from_numpy(buf), desc, 224, 224)
    assert _lib.load().ds_preprocess_train(None, 4, None, 1, None, None, 224, 224, None) == -1
    assert b"ds_preprocess_train" in _lib.load().ds_last_error()
