"""The host half of the JPEG decode against Pillow, byte for byte, without a GPU: ds_jpeg_probe + ds_jpeg_entropy_decode +
ds_jpeg_reconstruct_host over a grid of sizes x subsamplings x qualities x contents x crop boxes; restart intervals; streams
outside the supported set (they probe as unsupported and the loader's path returns PIL's pixels, or raises what PIL raises);
the compiled tf.Example reader against datasets.tfrecord.decode_example.  Images are generated from seeds with PIL."""
import io
import os

import numpy as np
import pytest
from PIL import Image

from tumblr_emotions_amd import _lib, ops
from tumblr_emotions_amd.input_pipeline import JpegCoefs, crop_box, decode_jpeg_bytes, decode_pixels

# odd sizes and one-past-a-block sizes: the smallest shapes at which the chroma edge and the padding blocks can go wrong
SIZES = ((1, 1), (7, 5), (8, 8), (15, 17), (16, 16), (17, 33), (31, 30), (48, 64), (75, 100))
SUBSAMPLINGS = (0, 1, 2, "L")
QUALITIES = (30, 90, 100)
CONTENTS = ("noise", "gradient", "constant")


def pixels(h, w, content, seed=0):
    rng = np.random.RandomState(seed * 7919 + h * 1000 + w)
    if content == "noise":                       # exercises saturation
        return rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
    if content == "gradient":
        yy, xx = np.mgrid[0:h, 0:w]
        return np.stack([yy * 255 // max(h - 1, 1), xx * 255 // max(w - 1, 1), (yy + xx) * 255 // max(h + w - 2, 1)],
                        -1).astype(np.uint8)
    return np.full((h, w, 3), (200, 30, 90), np.uint8)


def encode(a, subsampling, quality, **kw):
    bio = io.BytesIO()
    if subsampling == "L":
        Image.fromarray(a).convert("L").save(bio, "JPEG", quality=quality, **kw)
    else:
        Image.fromarray(a).save(bio, "JPEG", quality=quality, subsampling=subsampling, **kw)
    return bio.getvalue()


def pil_rgb(data):
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def boxes(h, w):
    """the full image, the loader's central crop, 1 x 1 crops at the four corners"""
    return [(0, 0, h, w), crop_box(h, w), (0, 0, 1, 1), (0, w - 1, 1, 1), (h - 1, 0, 1, 1), (h - 1, w - 1, 1, 1)]


_GRID = None


def grid():
    """[(label, jpeg bytes, PIL's RGB pixels)] of the baseline grid, built once per process."""
    global _GRID
    if _GRID is None:
        _GRID = []
        for h, w in SIZES:
            for sub in SUBSAMPLINGS:
                for q in QUALITIES:
                    for content in CONTENTS:
                        data = encode(pixels(h, w, content), sub, q)
                        _GRID.append(("%dx%d-%s-q%d-%s" % (h, w, sub, q, content), data, pil_rgb(data)))
    return _GRID


def decode_all(items):
    """Probe + entropy-decode [(label, data, ref)], one descriptor per (image, crop box), every descriptor with coefficient
    storage of its own: (coef int16, descriptors, byte count, [(label, box, byte offset, expected crop)]).  Sentinel-friendly:
    crops are laid out as pack_ragged lays them out (starts rounded up to 4 bytes)."""
    coefs, descs, expect, cpos, pos = [], [], [], 0, 0
    for label, data, ref in items:
        info = ops.jpeg_probe(data)
        assert info is not None, "the decoder reports a stream of the supported set as unsupported: " + label
        coef = ops.jpeg_entropy_decode(data, info)
        assert coef is not None, label
        h, w = ref.shape[:2]
        assert (info.height, info.width, info.coef_count) == (h, w, 64 * ops.jpeg_blocks(h, w, info.sampling)), label
        for box in boxes(h, w):
            y0, x0, ch, cw = box
            d = np.zeros((), ops.jpeg_desc_dtype())
            d["coef_offset"], d["out_offset"], d["width"], d["height"], d["sampling"] = cpos, pos, w, h, info.sampling
            d["y0"], d["x0"], d["crop_h"], d["crop_w"] = box
            d["quant"] = ops.jpeg_quant(info)
            descs.append(d)
            coefs.append((cpos, coef))
            expect.append((label, box, pos, ref[y0:y0 + ch, x0:x0 + cw]))
            cpos = -(-(cpos + coef.size) // 8) * 8
            pos = -(-(pos + ch * cw * 3) // 4) * 4
    all_coef = np.zeros(cpos, np.int16)
    for off, c in coefs:
        all_coef[off:off + c.size] = c
    return all_coef, np.asarray(descs, ops.jpeg_desc_dtype()), pos, expect


def check_bytes(out, nbytes, expect, sentinel=None):
    """Every crop equals PIL's; with `sentinel`, every byte outside the crops (gaps, the margins) still holds it."""
    untouched = np.ones(out.size, bool)
    for label, box, off, ref in expect:
        got = out[off:off + ref.size].reshape(ref.shape)
        assert np.array_equal(got, ref), (label, box, int(np.abs(got.astype(int) - ref).max()))
        untouched[off:off + ref.size] = False
    if sentinel is not None:
        assert (out[untouched] == sentinel).all()


def test_host_decoder_equals_pillow_on_the_whole_grid():
    items = grid()
    assert len(items) == len(SIZES) * len(SUBSAMPLINGS) * len(QUALITIES) * len(CONTENTS)
    coef, desc, nbytes, expect = decode_all(items)          # asserts that NO stream of the grid is reported unsupported
    assert len(desc) == 6 * len(items)
    out = np.full(nbytes + 64, 0xA5, np.uint8)
    desc["out_offset"] += 32
    ops.jpeg_reconstruct_host(coef, desc, out)
    check_bytes(out, nbytes, [(l, b, off + 32, r) for l, b, off, r in expect], sentinel=0xA5)


def test_sampling_classes_and_tables_are_the_headers():
    a = pixels(17, 33, "noise")
    for sub in SUBSAMPLINGS:
        info = ops.jpeg_probe(encode(a, sub, 90))
        assert info.sampling == (_lib.DS_JPEG_GREY if sub == "L" else sub) and info.components == (1 if sub == "L" else 3)
        assert info.restart_interval == 0 and info.coef_bytes == 2 * info.coef_count
    data = encode(a, 2, 75)
    q = Image.open(io.BytesIO(data)).quantization              # Pillow: zigzag order, table id -> 64 values
    zz = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21,
          28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54,
          47, 55, 62, 63]
    tables = ops.jpeg_quant(ops.jpeg_probe(data))
    for comp, tid in ((0, 0), (1, 1), (2, 1)):
        nat = np.zeros(64, np.int64)
        nat[zz] = np.asarray(q[tid])
        # Pillow >= 8.3 hands the tables out de-zigzagged already: accept whichever order it uses, the pixels are the arbiter
        assert np.array_equal(tables[comp], nat) or np.array_equal(tables[comp], np.asarray(q[tid])), comp


def _restart_kw():
    a = pixels(48, 64, "noise")
    for kw in ({"restart_marker_blocks": 3}, {"restart_marker_rows": 1}):
        try:
            data = encode(a, 2, 90, **kw)
        except TypeError:
            return None
        if b"\xff\xdd" not in data:
            return None
    return True


@pytest.mark.skipif(_restart_kw() is None, reason="this Pillow writes no restart markers (restart_marker_blocks / _rows)")
@pytest.mark.parametrize("kw", ({"restart_marker_blocks": 1}, {"restart_marker_blocks": 3}, {"restart_marker_blocks": 11},
                                {"restart_marker_rows": 1}, {"restart_marker_rows": 2}))
def test_restart_intervals(kw):
    items = []
    for h, w in ((17, 33), (48, 64), (75, 100)):
        for sub in SUBSAMPLINGS:
            data = encode(pixels(h, w, "noise", seed=3), sub, 90, **kw)
            info = ops.jpeg_probe(data)
            assert info is not None and info.restart_interval > 0, (h, w, sub, kw)
            items.append(("%dx%d-%s-%r" % (h, w, sub, kw), data, pil_rgb(data)))
    coef, desc, nbytes, expect = decode_all(items)
    out = np.zeros(nbytes, np.uint8)
    ops.jpeg_reconstruct_host(coef, desc, out)
    check_bytes(out, nbytes, expect)


def _loader_path_equals_pil(data, expect_fallback):
    """decode_jpeg_bytes (what a worker runs per image) against decode_pixels (today's path): the same pixels or the same
    exception."""
    try:
        want = decode_pixels(data)
    except Exception as e:             # noqa: BLE001 -- whatever PIL raises is what the loader must raise
        with pytest.raises(type(e)):
            decode_jpeg_bytes(data)
        return
    got = decode_jpeg_bytes(data)
    assert isinstance(got, JpegCoefs) != expect_fallback
    if expect_fallback:
        assert np.array_equal(got, want)


def test_unsupported_streams_probe_as_unsupported_and_fall_back_to_pil():
    a = pixels(48, 64, "gradient")
    streams = {}
    bio = io.BytesIO()
    Image.fromarray(a).save(bio, "JPEG", quality=90, progressive=True)
    streams["progressive"] = bio.getvalue()
    bio = io.BytesIO()
    Image.fromarray(a).convert("CMYK").save(bio, "JPEG", quality=90)
    streams["cmyk"] = bio.getvalue()
    # (Pillow writes no true 4:1:1 file: its "4:1:1" keyword is 4:2:0, which the grid covers)
    for name, data in streams.items():
        assert ops.jpeg_probe(data) is None, name
        _loader_path_equals_pil(data, expect_fallback=True)
    assert ops.jpeg_probe(b"") is None and ops.jpeg_probe(b"\xff\xd8") is None and ops.jpeg_probe(b"not a jpeg at all") is None


def test_every_truncated_file_of_the_grid_is_unsupported():
    for label, data, _ in grid():
        for frac in (0.25, 0.5, 0.75):
            cut = data[:int(len(data) * frac)]
            assert ops.jpeg_probe(cut) is None, (label, frac)
    for label, data, _ in grid():
        for frac in (0.25, 0.5, 0.75):
            _loader_path_equals_pil(data[:int(len(data) * frac)], expect_fallback=True)
    # damage inside the entropy-coded data that the marker walk cannot see: the Huffman decoder reports it
    label, data, _ = [g for g in grid() if g[0] == "48x64-2-q90-noise"][0]
    info = ops.jpeg_probe(data)
    short = data[:len(data) - 40] + data[-2:]               # 38 bytes of scan data gone, EOI in place
    if ops.jpeg_probe(short) is not None:
        assert ops.jpeg_entropy_decode(short, ops.jpeg_probe(short)) is None
    assert ops.jpeg_entropy_decode(data, info) is not None


def _with_quantisers(data, k):
    """The stream with every entry of every DQT table rewritten to k (8-bit tables)."""
    b, i = bytearray(data), 2
    while b[i + 1] != 0xDA:
        n = (b[i + 2] << 8) | b[i + 3]
        if b[i + 1] == 0xDB:
            for o in range(i + 4, i + 2 + n, 65):
                b[o + 1:o + 65] = bytes([k]) * 64
        i += 2 + n
    return bytes(b)


@pytest.mark.parametrize("sub", (0, 1, 2, "L"))
def test_rewritten_quantisers_give_pillows_bytes_or_a_fallback(sub):
    """libjpeg-turbo's SIMD inverse DCT forms some sums in 16 bits, so coefficients far beyond what pixels produce wrap
    there; the decoder must not accept a block it would reconstruct differently.  Quantisers of a quality-100 noise image
    are rewritten to a constant K: every K decodes to Pillow's bytes or is reported unsupported, K = 1 (the file as
    written, up to its tables) is supported, and K = 255 -- dequantised coefficients of thousands in every column, over the
    bound -- is not."""
    base = encode(pixels(64, 64, "noise", seed=9), sub, 100)
    outcomes = {}
    for k in list(range(1, 41)) + [64, 128, 255]:
        data = _with_quantisers(base, k)
        info = ops.jpeg_probe(data)
        assert info is not None, k                               # the markers are intact: the bound is the entropy decoder's
        coef = ops.jpeg_entropy_decode(data, info)
        outcomes[k] = coef is not None
        if coef is None:
            assert np.array_equal(decode_jpeg_bytes(data), decode_pixels(data)), k      # the loader's path: PIL's crop
            continue
        ref = pil_rgb(data)
        d = np.zeros(1, ops.jpeg_desc_dtype())
        d["width"], d["height"], d["sampling"], d["crop_h"], d["crop_w"] = 64, 64, info.sampling, 64, 64
        d["quant"][0] = ops.jpeg_quant(info)
        out = np.zeros(ref.size, np.uint8)
        ops.jpeg_reconstruct_host(coef, d, out)
        assert np.array_equal(out.reshape(ref.shape), ref), k
    assert outcomes[1] and not outcomes[255]
    first = min(k for k, ok in outcomes.items() if not ok)
    assert all(not ok for k, ok in outcomes.items() if k >= first)      # the bound is monotone in the quantiser


def test_oversized_headers_and_repeated_keys():
    """A header that claims more blocks than its scan can hold (or more pixels than Pillow's MAX_IMAGE_PIXELS) is
    unsupported at the probe, before anybody allocates for it; a repeated 'text' key leaves the LAST list, whole."""
    label, data, _ = grid()[-1]
    at = data.index(b"\xff\xc0") + 5
    assert ops.jpeg_probe(data[:at] + b"\xff\xff\xff\xff" + data[at + 4:]) is None          # 65535 x 65535
    assert ops.jpeg_probe(data[:at] + b"\x04\x00\x04\x00" + data[at + 4:]) is None          # 1024 x 1024 over a 75 x 100 scan
    from tumblr_emotions_amd.datasets.tfrecord import _len_field, _varint, decode_example

    def entry(name, ids):
        feat = _len_field(3, _len_field(1, b"".join(_varint(i) for i in ids)))
        return _len_field(1, _len_field(1, name) + _len_field(2, feat))

    body = entry(b"text", [9, 8, 7, 6, 5]) + entry(b"text", [1, 2]) + _len_field(
        1, _len_field(1, b"image/encoded") + _len_field(2, _len_field(1, _len_field(1, b"x"))))
    rec = _len_field(1, body)
    assert decode_example(rec)["text"] == [1, 2]
    got = ops.example_parse(rec)
    assert got is not None and got[2].tolist() == [1, 2] + [0] * (ops.JPEG_TEXT_CAPACITY - 2)


def test_good_streams_take_the_compiled_path_with_the_crop_made_from_the_header():
    for label, data, ref in grid()[::17]:
        got = decode_jpeg_bytes(data)
        assert isinstance(got, JpegCoefs), label
        assert (got.height, got.width) == ref.shape[:2] and got.box == crop_box(*ref.shape[:2])
    from tumblr_emotions_amd.preprocessing.inception_preprocessing import record_rng, sample_train_params
    label, data, ref = grid()[-1]
    got = decode_jpeg_bytes(data, train_key=(5, 1, 7))
    want = sample_train_params(ref.shape[0], ref.shape[1], record_rng(5, 1, 7))
    assert got.params == want and got.box == (want.y0, want.x0, want.crop_h, want.crop_w)


def test_check_jpeg_descs_rejects_what_the_kernel_cannot_report():
    coef, desc, nbytes, _ = decode_all(grid()[:2])
    ops.check_jpeg_descs(desc, coef.size, nbytes)
    for field, value in (("sampling", 4), ("crop_w", 0), ("x0", 10 ** 6), ("coef_offset", 4), ("out_offset", 2),
                         ("coef_offset", coef.size), ("out_offset", nbytes)):
        bad = desc.copy()
        bad[field][1] = value
        with pytest.raises(ValueError):
            ops.check_jpeg_descs(bad, coef.size, nbytes)
    bad = desc.copy()
    bad["out_offset"][1] = bad["out_offset"][0]              # two crops on the same bytes
    with pytest.raises(ValueError, match="overlap"):
        ops.check_jpeg_descs(bad, coef.size, nbytes)
    with pytest.raises(ValueError):
        ops.check_jpeg_descs(np.zeros(0, ops.jpeg_desc_dtype()), coef.size, nbytes)


@pytest.mark.parametrize("name", ("handmade_examples.tfrecord", "protobuf_examples.tfrecord"))
def test_compiled_example_reader_equals_decode_example(name):
    from tumblr_emotions_amd.datasets.tfrecord import decode_example, read_records
    path = os.path.join(os.path.dirname(__file__), "golden", name)
    taken = 0
    for rec in read_records(path):
        ex = decode_example(rec)
        ints = ("seq_len", "image/class/label", "post_id", "day")
        takes = (len(ex.get("image/encoded", [])) >= 1 and all(len(ex[k]) >= 1 for k in ints if k in ex)
                 and len(ex.get("text", [])) <= ops.JPEG_TEXT_CAPACITY
                 and all(isinstance(v, int) for k in ints + ("text",) for v in ex.get(k, [])))
        got = ops.example_parse(bytes(rec))
        assert (got is not None) == takes, ex.keys()
        if got is None:
            continue
        taken += 1
        off, length, text, seq_len, label, post_id, day = got
        assert bytes(rec[off:off + length]) == ex["image/encoded"][0]
        want = np.zeros(ops.JPEG_TEXT_CAPACITY, np.int64)
        want[:len(ex.get("text", []))] = ex.get("text", [])
        assert np.array_equal(text, want)
        assert [seq_len, label, post_id, day] == [ex.get(k, [0])[0] for k in ints]
    assert taken >= 1


def test_record_decode_is_one_call_and_asks_for_room():
    from tumblr_emotions_amd.datasets.tfrecord import encode_example
    from tumblr_emotions_amd.input_pipeline import decode_record, decode_record_jpeg
    label, data, ref = grid()[-1]
    rec = encode_example({"image/encoded": data, "image/format": b"jpg", "text": [3, 1, 4, 1, 5], "seq_len": 5,
                          "image/class/label": 2, "post_id": -77, "day": 9})
    r = ops.jpeg_record_decode(rec, np.empty(8, np.int16))
    assert r[0] == _lib.DS_JPEG_MORE and r[1].coef_count == 64 * ops.jpeg_blocks(75, 100, r[1].sampling)
    buf = np.empty(int(r[1].coef_count), np.int16)
    r = ops.jpeg_record_decode(rec, buf)
    assert r[0] == 0 and np.array_equal(buf, ops.jpeg_entropy_decode(data, ops.jpeg_probe(data)))
    want = decode_record(rec)
    got = decode_record_jpeg(rec)
    assert isinstance(got[0], JpegCoefs) and np.array_equal(got[1], want[1]) and got[2:] == want[2:]
    bio = io.BytesIO()
    Image.fromarray(ref).save(bio, "JPEG", progressive=True)
    rec = encode_example({"image/encoded": bio.getvalue(), "text": [1], "seq_len": 1, "image/class/label": 0, "post_id": 1, "day": 0})
    want, got = decode_record(rec), decode_record_jpeg(rec)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2:] == want[2:]
    with pytest.raises(KeyError):                  # no image: the Python parser's exception, as today
        decode_record_jpeg(encode_example({"text": [1]}))


def test_switch_is_refused_where_it_cannot_apply():
    from tumblr_emotions_amd.image_model.im_model import load_batch_with_text
    with pytest.raises(ValueError, match="jpeg_decode"):
        load_batch_with_text(None, pipeline="host", jpeg_decode="device")
    with pytest.raises(ValueError, match="jpeg_decode"):
        load_batch_with_text(None, pipeline="device", jpeg_decode="gpu")
    from tumblr_emotions_amd.training import SyntheticInput
    with pytest.raises(ValueError, match="jpeg_decode"):
        SyntheticInput()._init_input({"jpeg_decode": "device", "synthetic": True}, 50, 10, 3, True, "cpu")
