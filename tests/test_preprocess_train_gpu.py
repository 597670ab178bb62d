"""ds_preprocess_train against the package's NumPy preprocess_for_train, bit for bit (np.array_equal, no tolerance: both
sides are the same sequence of single fp32 roundings): every element of every image, the eval kernel test's sizes and
output sizes crossed with a parameter set, branch-hitting images, ragged launches, B = 256, sentinels around the output."""
import numpy as np
import pytest
import torch

from tumblr_emotions_amd import input_pipeline as P
from tumblr_emotions_amd import ops
from tumblr_emotions_amd.preprocessing import inception_preprocessing as ip

pytestmark = pytest.mark.gpu

FIXED_SIZES = [(1, 1), (7, 3), (224, 224), (256, 256), (333, 499), (375, 500), (50, 1000), (1500, 2000)]
OUTS = (224, 299)
PAD = 1024
SENTINEL = -12345.5
F = np.float32
DELTAS = (F(-32 / 255), F(0), F(32 / 255))
FACTORS = (F(0), F(0.5), F(1), F(1.4999))
# every (delta, factor) pair once; flip and the colour order vary so that each pairs with every delta and every factor
PARAM_SET = [(bool((i + j) & 1), bool(((i + 2 * j) >> 1) & 1), d, f) for i, d in enumerate(DELTAS) for j, f in enumerate(FACTORS)]


def _random_sizes():
    rng = np.random.RandomState(20)
    return [(int(h), int(w)) for h, w in rng.randint(8, 1201, size=(20, 2))]


def _image(h, w, seed):
    return np.random.RandomState(seed).randint(0, 256, size=(h, w, 3)).astype(np.uint8)


def _whole(im, flip, sat_first, delta, factor):
    return ip.TrainParams(0, 0, im.shape[0], im.shape[1], flip, sat_first, F(delta), F(factor))


def _device(images, params, out_h, out_w, share=False):
    """One launch over the crops of `images` (full uint8 arrays) described by `params`: slice on the host, pack, preprocess
    into a buffer with sentinel floats on both sides, check the sentinels, return [B, out_h, out_w, 3] as NumPy.
    share=True: `images` is ONE image and every parameter set reads the same packed bytes (descriptors may overlap)."""
    crops = [np.ascontiguousarray(im[p.y0:p.y0 + p.crop_h, p.x0:p.x0 + p.crop_w]) for im, p in zip(images, params)]
    if share:
        buf, one, used = P.pack_ragged(crops[:1], out_h, out_w, params=params[:1])
        desc = np.zeros(len(params), ops.preprocess_train_desc_dtype())
        for i, p in enumerate(params):
            assert (p.y0, p.x0, p.crop_h, p.crop_w) == tuple(params[0][:4])
            desc[i] = P.pack_ragged(crops[:1], out_h, out_w, params=[p])[1][0]
    else:
        buf, desc, used = P.pack_ragged(crops, out_h, out_w, params=params)
    B = len(params)
    n = B * out_h * out_w * 3
    guard = torch.full((n + 2 * PAD,), SENTINEL, dtype=torch.float32, device="cuda")
    out = guard[PAD:PAD + n].view(B, out_h, out_w, 3)
    got = ops.preprocess_train(torch.from_numpy(buf[:max(used, 4)]).cuda(), desc, out_h, out_w, out=out)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr()
    g = guard.cpu().numpy()
    assert (g[:PAD] == np.float32(SENTINEL)).all() and (g[PAD + n:] == np.float32(SENTINEL)).all(), "sentinels overwritten"
    return g[PAD:PAD + n].reshape(B, out_h, out_w, 3)


def _check(images, params, out_h, out_w, share=False):
    got = _device(images, params, out_h, out_w, share)
    for i, p in enumerate(params):
        im = images[0] if share else images[i]
        want = ip.preprocess_for_train(im, out_h, out_w, p)
        assert want.dtype == np.float32 and want.shape == got[i].shape
        assert np.array_equal(got[i], want), ("image %d of %d, %s, %s -> %dx%d: %d elements differ, max |d| = %g"
                                              % (i, len(params), im.shape, p, out_h, out_w, int((got[i] != want).sum()),
                                                 float(np.abs(got[i] - want).max())))


@pytest.mark.parametrize("out", OUTS)
@pytest.mark.parametrize("size", FIXED_SIZES + _random_sizes(), ids=lambda s: "%dx%d" % s)
def test_every_parameter_set_is_bit_identical(size, out):
    im = _image(size[0], size[1], seed=size[0] * 7919 + size[1])
    _check([im] * len(PARAM_SET), [_whole(im, *q) for q in PARAM_SET], out, out, share=True)


def _branch_image():
    """Pixels that take every branch of the saturation code: grey (range = 0), black, white, r = g = max and g = b = max
    ties, each channel the strict maximum with either order of the other two (h < 0 when r is the maximum and g < b),
    near-grey pixels one step apart, saturated primaries and secondaries; then uniform noise."""
    px = [(0, 0, 0), (255, 255, 255), (128, 128, 128), (1, 1, 1), (200, 200, 10), (10, 200, 200), (200, 10, 200),
          (200, 50, 100), (200, 100, 50), (50, 200, 100), (100, 200, 50), (50, 100, 200), (100, 50, 200),
          (128, 127, 127), (127, 128, 127), (127, 127, 128), (255, 254, 255), (255, 0, 0), (0, 255, 0), (0, 0, 255),
          (255, 255, 0), (0, 255, 255), (255, 0, 255), (255, 0, 1), (1, 0, 0), (0, 1, 0), (0, 0, 1), (254, 255, 255)]
    rows = np.array(px, np.uint8)
    im = np.concatenate([np.repeat(rows[None], 12, axis=0),
                         np.random.RandomState(4).randint(0, 256, size=(12, len(px), 3)).astype(np.uint8)], axis=0)
    return np.ascontiguousarray(im)


@pytest.mark.parametrize("out", ("same",) + OUTS)
def test_branch_hitting_images(out):
    """out = 'same': the scales are 1, so every pixel passes through the resize unchanged and meets the colour chain as built;
    the other sizes blend neighbouring special pixels."""
    im = _branch_image()
    oh, ow = im.shape[:2] if out == "same" else (out, out)
    full = [(fl, sf, d, f) for fl in (False, True) for sf in (False, True) for d in DELTAS for f in FACTORS]
    _check([im] * len(full), [_whole(im, *q) for q in full], oh, ow, share=True)
    for value in (0, 255, 77):
        const = np.full((9, 14, 3), value, np.uint8)
        _check([const] * len(PARAM_SET), [_whole(const, *q) for q in PARAM_SET], oh, ow, share=True)


@pytest.mark.parametrize("out", OUTS)
def test_constant_images_with_full_brightness_give_exactly_plus_and_minus_one(out):
    for value, delta, expect in ((255, 32 / 255, 1.0), (0, -32 / 255, -1.0)):
        im = np.full((60, 31, 3), value, np.uint8)
        got = _device([im, im], [_whole(im, False, False, delta, 1.2), _whole(im, True, True, delta, 0.7)], out, out)
        assert (got == np.float32(expect)).all()


@pytest.mark.parametrize("out", OUTS)
def test_one_ragged_launch_with_sampled_parameters_per_image(out):
    sizes = FIXED_SIZES + _random_sizes()
    images = [_image(h, w, seed=1000 + i) for i, (h, w) in enumerate(sizes)]
    images += [np.zeros((40, 30, 3), np.uint8), np.full((30, 40, 3), 255, np.uint8), _branch_image()]
    params = [ip.sample_train_params(im.shape[0], im.shape[1], ip.record_rng(out, 0, i)) for i, im in enumerate(images)]
    assert len({(p.flip, p.saturation_first) for p in params}) == 4
    assert any(p[:4] != (0, 0) + im.shape[:2] for p, im in zip(params, images))
    _check(images, params, out, out)


def test_rectangular_output():
    ims = [_image(375, 500, 1), _image(100, 37, 2)]
    _check(ims, [ip.TrainParams(20, 30, 300, 400, True, True, F(0.05), F(1.3)), _whole(ims[1], True, False, -0.1, 0.6)], 224, 299)


def test_batch_of_256():
    rng = np.random.RandomState(256)
    images = [_image(int(h), int(w), seed=5000 + i) for i, (h, w) in enumerate(rng.randint(8, 161, size=(256, 2)))]
    params = [ip.sample_train_params(im.shape[0], im.shape[1], ip.record_rng(256, 1, i)) for i, im in enumerate(images)]
    _check(images, params, 224, 224)


def test_bad_arguments_are_rejected_before_any_launch():
    im = _image(20, 20, 0)
    buf, desc, used = P.pack_ragged([im], 224, 224, params=[_whole(im, False, True, 0.1, 1.0)])
    dev = torch.from_numpy(buf).cuda()
    for field, value, msg in (("height", 21, "does not fit"), ("delta", np.inf, "finite"), ("factor", np.nan, "finite"),
                              ("factor", -1.0, "factor"), ("flags", 8, "flag"), ("reserved", 3, "flag"), ("scale_y", -1.0, "scales")):
        bad = desc.copy()
        bad[field][0] = value
        with pytest.raises(ValueError, match=msg):
            ops.preprocess_train(dev, bad, 224, 224)
    with pytest.raises(ValueError):
        ops.preprocess_train(dev, desc, 0, 224)
    with pytest.raises(ValueError):
        ops.preprocess_train(dev, P.pack_ragged([im], 224, 224)[1], 224, 224)        # eval records
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.preprocess_train(torch.from_numpy(buf), desc, 224, 224)
    from tumblr_emotions_amd import _lib
    assert _lib.load().ds_preprocess_train(None, 4, None, 1, None, None, 224, 224, None) == -1
    ops.preprocess_train(dev, desc, 224, 224)                                        # the good one runs
    torch.cuda.synchronize()
