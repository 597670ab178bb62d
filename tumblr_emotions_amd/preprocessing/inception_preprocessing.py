"""`preprocess_for_eval` of slim/preprocessing/inception_preprocessing.py:237-275 in NumPy -- the ONLY
image pipeline the reference's training path uses (load_batch_with_text is always called with
is_training=False, image_model/im_model.py:78,102): uint8 -> [0,1] float, central crop 87.5 %, bilinear
resize (align_corners=False, TF-1.x legacy sampling src = dst * in/out), then (x - 0.5) * 2.

[TF-sem] tf.image.central_crop: start = int((size - size*fraction) / 2), extent = size - 2*start.
Parity unpinned: no TensorFlow output is available to compare the resize against.

`preprocess_for_train` (:156-234, reached through preprocess_image(is_training=True), :278-304) with the defaults its call
site leaves (bbox=None, fast_mode=True), summaries dropped:
    v / 255 -> distorted_bounding_box_crop (whole image as the only box: min_object_covered 0.1, aspect_ratio_range
    (0.75, 1.33), area_range (0.05, 1.0), max_attempts 100) -> bilinear resize (fast mode: the one method) ->
    random_flip_left_right -> distort_color(fast_mode=True): ordering 0 = brightness (delta ~ U[-32/255, 32/255)) then
    saturation (factor ~ U[0.5, 1.5)), orderings 1-3 = saturation then brightness; clip to [0, 1] -> (x - 0.5) * 2.
The random draws are separated from the arithmetic: `sample_train_params` draws everything an image needs from a generator,
`preprocess_for_train` is a pure function of the image and those parameters, every operation ONE fp32 rounding in the
order written here, so that the HIP kernel ds_preprocess_train repeats it bit for bit.

[TF-sem] Two pieces are TensorFlow C++ kernels, restated here from memory, parity unpinned:
  * the crop sampler (GenerateRandomCrop of sample_distorted_bounding_box_op.cc), see sample_distorted_crop;
  * the fused AdjustSaturation CPU kernel (RGB -> HSV, S scaled and clamped, HSV -> RGB in fp32), see adjust_saturation.
    Its constants 2/6 and 4/6 are taken as fp32 values and every operation as one fp32 rounding.
TensorFlow's random stream (Philox behind graph seeds) is not reproduced and nothing pins it: the contract is the
DISTRIBUTIONS above and the stream of `record_rng`, which depends on (seed, pass, global record index) only -- never on the
worker count, the thread timing or the data-parallel world size -- and is shared by the host and the device pipeline."""
import collections
import math

import numpy as np


def central_crop(image, central_fraction):
    h, w = image.shape[0], image.shape[1]
    h0 = int((h - h * central_fraction) / 2)
    w0 = int((w - w * central_fraction) / 2)
    return image[h0:h0 + (h - 2 * h0), w0:w0 + (w - 2 * w0)]


def resize_bilinear(image, height, width):
    """[H,W,C] float32 -> [height,width,C]; tf.image.resize_bilinear(align_corners=False), TF 1.x."""
    h, w = image.shape[0], image.shape[1]

    def axis(n_in, n_out):
        src = np.arange(n_out, dtype=np.float32) * np.float32(n_in / n_out)
        lo = np.floor(src).astype(np.int64)
        hi = np.minimum(lo + 1, n_in - 1)
        return lo, hi, (src - lo).astype(np.float32)

    y0, y1, fy = axis(h, height)
    x0, x1, fx = axis(w, width)
    top = image[y0][:, x0] + (image[y0][:, x1] - image[y0][:, x0]) * fx[None, :, None]
    bot = image[y1][:, x0] + (image[y1][:, x1] - image[y1][:, x0]) * fx[None, :, None]
    return (top + (bot - top) * fy[:, None, None]).astype(np.float32)


def preprocess_for_eval(image, height, width, central_fraction=0.875):
    if image.dtype != np.float32:
        image = image.astype(np.float32) / np.float32(np.iinfo(image.dtype).max)     # convert_image_dtype
    if central_fraction:
        image = central_crop(image, central_fraction)
    if height and width:
        image = resize_bilinear(image, height, width)
    return (image - np.float32(0.5)) * np.float32(2.0)


# ---- train-time augmentation ------------------------------------------------------------------------------------------------
MAX_ATTEMPTS = 100
MIN_OBJECT_COVERED = 0.1
ASPECT_RATIO_RANGE = (0.75, 1.33)
AREA_RANGE = (0.05, 1.0)
MAX_BRIGHTNESS_DELTA = 32.0 / 255.0
SATURATION_RANGE = (0.5, 1.5)
_FIRST_ATTEMPTS = 8          # variates of the first attempts are drawn in one call; the other 92 only when all of these fail

TrainParams = collections.namedtuple("TrainParams", "y0 x0 crop_h crop_w flip saturation_first delta factor")


def record_rng(seed, pass_no, index):
    """The generator of ONE record's augmentation draws: Philox keyed by (seed, pass number), its 256-bit counter started
    at index * 2**64 -- a function of (seed, pass, global record index within the pass) and of nothing else.  Both input
    pipelines call this where they submit a record; streams of different records never overlap."""
    mask = (1 << 64) - 1
    return np.random.Generator(np.random.Philox(counter=[0, int(index) & mask, 0, 0],
                                                key=[int(seed or 0) & mask, int(pass_no) & mask]))


def _lrint(x):
    return int(round(x))         # round half to even, as lrint in the default rounding mode


def _crop_attempt(h_img, w_img, u_aspect, u_h, u_y, u_x):
    """One attempt of GenerateRandomCrop from four uniforms in [0, 1): (y0, x0, h, w), or None when rejected.
    randint(n) is int(u * n)."""
    aspect = ASPECT_RATIO_RANGE[0] + u_aspect * (ASPECT_RATIO_RANGE[1] - ASPECT_RATIO_RANGE[0])
    min_area = AREA_RANGE[0] * w_img * h_img
    max_area = AREA_RANGE[1] * w_img * h_img
    h_min = _lrint(math.sqrt(min_area / aspect))
    h_max = _lrint(math.sqrt(max_area / aspect))
    if _lrint(h_max * aspect) > w_img:
        h_max = int((w_img + 0.5 - 1e-7) / aspect)
    h_max = min(h_max, h_img)
    h = min(h_min, h_max)
    if h < h_max:
        h += min(int(u_h * (h_max - h + 1)), h_max - h)
    w = _lrint(h * aspect)
    if w * h < min_area:
        h += 1
        w = _lrint(h * aspect)
    if w * h > max_area:
        h -= 1
        w = _lrint(h * aspect)
    area = w * h
    if area < min_area or area > max_area or w > w_img or h > h_img or w <= 0 or h <= 0:
        return None
    y = min(int(u_y * (h_img - h)), h_img - h - 1) if h < h_img else 0
    x = min(int(u_x * (w_img - w)), w_img - w - 1) if w < w_img else 0
    if area < MIN_OBJECT_COVERED * w_img * h_img:          # the box is the whole image: coverage = area fraction
        return None
    return y, x, h, w


def _sample_crop(h, w, rng):
    """(box, attempts used); attempts == MAX_ATTEMPTS + 1 marks the whole-image fallback."""
    h, w = int(h), int(w)
    done = 0
    for n in (_FIRST_ATTEMPTS, MAX_ATTEMPTS - _FIRST_ATTEMPTS):
        u = rng.random(4 * n).tolist()
        for k in range(n):
            box = _crop_attempt(h, w, u[4 * k], u[4 * k + 1], u[4 * k + 2], u[4 * k + 3])
            if box is not None:
                return box, done + k + 1
        done += n
    return (0, 0, h, w), MAX_ATTEMPTS + 1


def sample_distorted_crop(h, w, rng):
    """[TF-sem] sample_distorted_bounding_box with the whole image as the only box -> (y0, x0, crop_h, crop_w).
    Per attempt: aspect ~ U[0.75, 1.33); h_min / h_max = lrint(sqrt(0.05 / 1.0 * W * H / aspect)); h_max is cut to what
    fits the width and the height; the height is uniform on [h_min, h_max], the width lrint(h * aspect), nudged by one row
    back into the area range; rejected when the area leaves [0.05, 1] * W * H or the box leaves the image; the corner is
    uniform on [0, H - h) x [0, W - w); accepted when the crop covers 0.1 of the image.  After 100 rejected attempts the
    whole image is the crop.  Draw order (part of the stream contract): the four uniforms (aspect, height, y, x) of
    attempts 1-8 in one rng.random(32) call; only if all eight are rejected those of attempts 9-100 in one
    rng.random(368) call."""
    return _sample_crop(h, w, rng)[0]


def sample_train_params(h, w, rng):
    """Every random choice preprocess_for_train needs for an h x w image, in ONE fixed draw order: the crop attempts
    (sample_distorted_crop), then one rng.random(4) call = flip, colour ordering, brightness delta, saturation factor.
    flip = u < 0.5; ordering = int(u * 4) with 0 = brightness first, 1-3 = saturation first; delta and factor are rounded
    to np.float32 once, here."""
    y0, x0, ch, cw = sample_distorted_crop(h, w, rng)
    u_flip, u_order, u_delta, u_factor = rng.random(4).tolist()
    delta = np.float32(-MAX_BRIGHTNESS_DELTA + u_delta * (2.0 * MAX_BRIGHTNESS_DELTA))
    factor = np.float32(SATURATION_RANGE[0] + u_factor * (SATURATION_RANGE[1] - SATURATION_RANGE[0]))
    return TrainParams(y0, x0, ch, cw, u_flip < 0.5, int(u_order * 4) != 0, delta, factor)


def adjust_saturation(image, factor):
    """[TF-sem] the fused AdjustSaturation kernel on an [..., 3] float32 image: RGB -> (h, s, v), s = clamp(s * factor, 0, 1),
    back to RGB -- every line below one fp32 rounding per element; divisors are selected before dividing, so nothing is
    divided by zero.  factor 1 is not the identity in fp32."""
    f32 = np.float32
    image = np.asarray(image, np.float32)
    r, g, b = image[..., 0], image[..., 1], image[..., 2]
    v = np.maximum(np.maximum(r, g), b)
    mn = np.minimum(np.minimum(r, g), b)
    rng_ = v - mn
    s = np.where(v > 0, rng_ / np.where(v > 0, v, f32(1)), f32(0))
    norm = f32(1) / np.where(rng_ > 0, f32(6) * rng_, f32(1))
    h = np.where(r == v, norm * (g - b), np.where(g == v, norm * (b - r) + f32(2.0 / 6.0), norm * (r - g) + f32(4.0 / 6.0)))
    h = np.where(rng_ <= 0, f32(0), h)
    h = np.where(h < 0, h + f32(1), h)
    s = np.minimum(f32(1), np.maximum(f32(0), s * f32(factor)))
    c = s * v
    m = v - c
    dh = h * f32(6)
    cat = dh.astype(np.int32)                                  # truncation; dh >= 0
    f = dh
    while True:
        low = f <= 0
        if not low.any():
            break
        f = np.where(low, f + f32(2), f)
    while True:
        high = f >= 2
        if not high.any():
            break
        f = np.where(high, f - f32(2), f)
    x = c * (f32(1) - np.abs(f - f32(1)))
    zero = np.zeros_like(c)
    rr = np.select([cat == 0, cat == 1, cat == 2, cat == 3, cat == 4, cat == 5], [c, x, zero, zero, x, c], zero)
    gg = np.select([cat == 0, cat == 1, cat == 2, cat == 3, cat == 4, cat == 5], [x, c, c, x, zero, zero], zero)
    bb = np.select([cat == 0, cat == 1, cat == 2, cat == 3, cat == 4, cat == 5], [zero, zero, x, c, c, x], zero)
    return np.stack([rr + m, gg + m, bb + m], axis=-1).astype(np.float32)


def distort_color_fast(image, saturation_first, delta, factor):
    """distort_color(fast_mode=True): brightness (image + delta) and saturation in the drawn order, then clip to [0, 1]."""
    f32 = np.float32
    image = np.asarray(image, np.float32)
    if saturation_first:
        image = adjust_saturation(image, factor) + f32(delta)
    else:
        image = adjust_saturation(image + f32(delta), factor)
    return np.minimum(np.maximum(image, f32(0)), f32(1))


def preprocess_for_train(image, height, width, params):
    """preprocess_for_train for already drawn `params` (a TrainParams): convert, slice the crop, resize, flip the RESIZED
    image, distort the colours, scale to [-1, 1]."""
    if image.dtype != np.float32:
        image = image.astype(np.float32) / np.float32(np.iinfo(image.dtype).max)     # convert_image_dtype
    p = params
    image = image[p.y0:p.y0 + p.crop_h, p.x0:p.x0 + p.crop_w]
    image = resize_bilinear(image, height, width)
    if p.flip:
        image = image[:, ::-1]
    image = distort_color_fast(image, p.saturation_first, p.delta, p.factor)
    return (image - np.float32(0.5)) * np.float32(2.0)


def preprocess_image(image, height, width, is_training=False, bbox=None, fast_mode=True, rng=None):
    """is_training=True: `rng` (a np.random.Generator, e.g. record_rng(...); a fresh default_rng() when None) supplies the
    draws of sample_train_params."""
    if not is_training:
        return preprocess_for_eval(image, height, width)
    if bbox is not None:
        raise NotImplementedError("caller-supplied bounding boxes are not implemented: the records carry none, the whole "
                                  "image is the box")
    if not fast_mode:
        raise NotImplementedError("fast_mode=False (hue, contrast, the bicubic / nearest / area resize methods) is not "
                                  "implemented: load_batch_with_text leaves fast_mode=True")
    if rng is None:
        rng = np.random.default_rng()
    return preprocess_for_train(image, height, width, sample_train_params(image.shape[0], image.shape[1], rng))
