"""Restart-segmented JPEGs without a GPU: the lossless restart transcoder (ds_jpeg_restart_transcode) against Pillow and
against ds_jpeg_entropy_decode over a grid of sizes x subsamplings x qualities x optimize x contents x intervals;
datasets.convert_to_dataset.add_restart_markers on a small dataset; and ds_jpeg_entropy_decode_segments_host -- the CPU
statement of the device launch, the shared lines of csrc/jpeg_common.h -- against ds_jpeg_entropy_decode: status 0 exactly
when that returns DS_OK, then all coefficients equal, and never a store outside an image's own range (guard bands).
Images are generated from seeds with PIL.  tests/test_jpeg_entropy_gpu.py runs the same streams through the kernel."""
import io
import os

import numpy as np
import pytest
from PIL import Image

from test_jpeg_cpu import SUBSAMPLINGS, _with_quantisers, encode, pil_rgb, pixels
from tumblr_emotions_amd import ops

T_SIZES = ((1, 1), (8, 8), (17, 33), (33, 17), (75, 100))          # (height, width)
T_QUALITIES = (30, 100)
T_CONTENTS = ("noise", "gradient", "constant")
T_INTERVALS = (0, 1, 3)
GUARD = 16                                               # int16 in front of, between and behind the images' ranges
PATTERN = 0x5A5A
RESTART_KW = ({"restart_marker_blocks": 1}, {"restart_marker_blocks": 3}, {"restart_marker_blocks": 11},
              {"restart_marker_rows": 1}, {"restart_marker_rows": 2},
              {"restart_marker_blocks": 5000})           # the last: an interval larger than any image's MCU count


def dht_tables(data):
    """{(class, id): (counts, values)} of the DHT segments in front of SOS."""
    out, i = {}, 2
    while data[i + 1] != 0xDA:
        n = (data[i + 2] << 8) | data[i + 3]
        if data[i + 1] == 0xC4:
            o = i + 4
            while o < i + 2 + n:
                total = sum(data[o + 1:o + 17])
                out[(data[o] >> 4, data[o] & 15)] = (bytes(data[o + 1:o + 17]), bytes(data[o + 17:o + 17 + total]))
                o += 17 + total
        i += 2 + n
    return out


def _check_transcode(src, data, interval, want_pixels, want_coef):
    out = ops.jpeg_restart_transcode(data, interval)
    assert out is not None, (src, interval)
    assert np.array_equal(pil_rgb(out), want_pixels), (src, interval)
    info = ops.jpeg_probe(out)
    assert info is not None, (src, interval)
    mw, _ = ops.jpeg_mcus(info.height, info.width, info.sampling)
    assert info.restart_interval == (interval or mw), (src, interval)
    assert np.array_equal(ops.jpeg_entropy_decode(out, info), want_coef), (src, interval)
    return out


@pytest.mark.parametrize("sub", SUBSAMPLINGS)
def test_transcoder_is_lossless_over_the_grid(sub):
    replaced = unchanged = 0
    for h, w in T_SIZES:
        for q in T_QUALITIES:
            for optimize in (False, True):
                for content in T_CONTENTS:
                    src = (h, w, sub, q, optimize, content)
                    data = encode(pixels(h, w, content), sub, q, optimize=optimize)
                    want_pixels = pil_rgb(data)
                    want_coef = ops.jpeg_entropy_decode(data, ops.jpeg_probe(data))
                    assert want_coef is not None, src
                    outs = [_check_transcode(src, data, iv, want_pixels, want_coef) for iv in T_INTERVALS]
                    # an already restart-marked file to another interval
                    _check_transcode(src, outs[2], 0, want_pixels, want_coef)
                    _check_transcode(src, outs[0], 1, want_pixels, want_coef)
                    for out in outs:
                        same = dht_tables(out) == dht_tables(data)
                        assert same or optimize, src        # the standard tables have every code: they always stay
                        replaced += not same
                        unchanged += same
    assert unchanged > 0
    if sub != "L":
        # a DC difference at a segment start is taken from zero, and an optimised table may lack that category: the table
        # is replaced (the DHT differs) and the pixels are still equal (asserted above for every case)
        assert replaced > 0, "no stream of the grid needed a replaced table: the case dropped out"


def test_a_replaced_dc_table_is_found_and_the_pixels_stay():
    found = []
    for content in T_CONTENTS:
        for sub in SUBSAMPLINGS:
            data = encode(pixels(75, 100, content), sub, 30, optimize=True)
            out = ops.jpeg_restart_transcode(data, 0)
            a, b = dht_tables(data), dht_tables(out)
            dc = [k for k in a if k[0] == 0 and a[k] != b[k]]
            if dc:
                found.append((content, sub))
                assert np.array_equal(pil_rgb(out), pil_rgb(data))
                for k in dc:                     # the replacement has a code for every category 0 .. 11
                    assert sorted(b[k][1]) == list(range(12))
    assert found, "no optimised stream needed a replaced DC table"


def test_transcoder_refuses_what_the_decoder_does_not_support():
    a = pixels(48, 64, "gradient")
    bio = io.BytesIO()
    Image.fromarray(a).save(bio, "JPEG", quality=90, progressive=True)
    assert ops.jpeg_restart_transcode(bio.getvalue()) is None
    bio = io.BytesIO()
    Image.fromarray(a).convert("CMYK").save(bio, "JPEG", quality=90)
    assert ops.jpeg_restart_transcode(bio.getvalue()) is None
    assert ops.jpeg_restart_transcode(b"") is None and ops.jpeg_restart_transcode(b"not a jpeg") is None
    with pytest.raises(ValueError):
        ops.jpeg_restart_transcode(encode(a, 2, 90), 65536)
    # the cost in file size: a DRI segment (6 bytes) and per MCU row a marker (2) and less than a byte of padding; one DHT
    # segment instead of Pillow's four gives 12 bytes back
    data = encode(pixels(75, 100, "noise"), 2, 90)
    out = ops.jpeg_restart_transcode(data)
    assert -12 <= len(out) - len(data) <= 6 + 3 * 5 - 12


def test_scan_reports_what_probe_reports_plus_tables_and_cuts():
    data = encode(pixels(75, 100, "noise", seed=3), 2, 90, restart_marker_rows=1)
    info, scan, cuts = ops.jpeg_scan(data)
    probe = ops.jpeg_probe(data)
    assert bytes(info) == bytes(probe)
    mw, mh = ops.jpeg_mcus(75, 100, info.sampling)
    assert scan.cut_count == cuts.size == mh and info.restart_interval == mw
    assert data[scan.scan_begin - 14:scan.scan_begin - 12] == b"\xff\xda" and data[cuts[-1]:cuts[-1] + 2] == b"\xff\xd9"
    for k, c in enumerate(cuts[:-1]):
        assert data[c] == 0xFF and data[c + 1] == 0xD0 + (k & 7)
    tables = dht_tables(data)
    for c, (td, ta) in enumerate(((0, 0), (1, 1), (1, 1))):
        assert bytes(scan.dc[c].counts) == tables[(0, td)][0] and bytes(scan.dc[c].values)[:12] == tables[(0, td)][1]
        assert bytes(scan.ac[c].counts) == tables[(1, ta)][0] and bytes(scan.ac[c].values)[:162] == tables[(1, ta)][1]
    bio = io.BytesIO()
    Image.fromarray(pixels(48, 64, "gradient")).save(bio, "JPEG", progressive=True)
    assert ops.jpeg_scan(bio.getvalue()) is None and ops.jpeg_scan(data[:300]) is None


def test_add_restart_markers_rewrites_only_the_supported_images(tmp_path):
    from tumblr_emotions_amd.datasets.convert_to_dataset import add_restart_markers
    from tumblr_emotions_amd.datasets.tfrecord import decode_example, encode_example, read_records, write_records
    src = tmp_path / "tfrecords"
    os.makedirs(str(src))
    originals = {}
    for shard in range(2):
        recs = []
        for i in range(shard * 4, shard * 4 + 4):
            a = pixels(40 + i, 30 + 2 * i, ("noise", "gradient")[i % 2], seed=i)
            bio = io.BytesIO()
            Image.fromarray(a).save(bio, "JPEG", quality=85, subsampling=i % 3, progressive=(i == 5))
            recs.append(encode_example({"image/encoded": bio.getvalue(), "image/format": b"jpg", "image/class/label": i % 3,
                                        "text": [i, i + 1, 7], "seq_len": 3, "post_id": -i, "day": i % 7, "score": [0.5, float(i)]}))
        name = "tumblr_train_%05d-of-00002.tfrecord" % shard
        write_records(str(src / name), recs)
        originals[name] = recs
    assert add_restart_markers(str(tmp_path)) == (7, 1)
    with pytest.raises(ValueError):
        add_restart_markers(str(tmp_path), out_subdir="tfrecords")
    for name, recs in originals.items():
        new = [bytes(r) for r in read_records(str(tmp_path / "tfrecords_rst" / name), verify=True)]
        assert len(new) == len(recs)
        for old_rec, new_rec in zip(recs, new):
            a, b = decode_example(old_rec), decode_example(new_rec)
            assert list(a) == list(b)
            for key in a:
                if key != "image/encoded":
                    assert a[key] == b[key], key
            old_img, new_img = a["image/encoded"][0], b["image/encoded"][0]
            if a["post_id"] == [-5]:                                  # the progressive file: its bytes, the record's bytes
                assert new_img == old_img and new_rec == old_rec
            else:
                info = ops.jpeg_probe(new_img)
                assert info.restart_interval == ops.jpeg_mcus(info.height, info.width, info.sampling)[0]
                assert np.array_equal(pil_rgb(new_img), pil_rgb(old_img))


# ---- the segment decoder against ds_jpeg_entropy_decode -------------------------------------------------------------------------
def tables_with_guards(datas):
    """(scan, images, segs, coefficient buffer size, [(offset, count)]) of a batch of encoded streams ds_jpeg_probe accepts:
    each image's range with GUARD int16 in front of and behind it."""
    streams = [(d,) + ops.jpeg_scan(d) for d in datas]
    offsets, cpos = [], GUARD
    for _, info, _, _ in streams:
        offsets.append(cpos)
        cpos = -(-(cpos + int(info.coef_count)) // 8) * 8 + GUARD
    scan, images, segs, _ = ops.make_jpeg_scan_tables(streams, offsets)
    return scan, images, segs, cpos, [(o, int(st[1].coef_count)) for o, st in zip(offsets, streams)]


def check_equivalence(datas, status, coef, ranges):
    """The equivalence contract for every image of a decoded batch; returns how many images were flagged."""
    outside = np.ones(coef.size, bool)
    flagged = 0
    for i, (data, (off, count)) in enumerate(zip(datas, ranges)):
        want = ops.jpeg_entropy_decode(data, ops.jpeg_probe(data))
        assert (status[i] == 0) == (want is not None), (i, int(status[i]))
        if want is not None:
            assert np.array_equal(coef[off:off + count], want), i
        flagged += want is None
        outside[off:off + count] = False
    assert (coef[outside] == PATTERN).all(), "a store outside the images' own coefficient ranges"
    return flagged


def decode_on_host(datas):
    scan, images, segs, ncoef, ranges = tables_with_guards(datas)
    coef = np.full(ncoef, PATTERN, np.int16)
    status = ops.jpeg_entropy_decode_segments_host(scan, images, segs, coef)
    return check_equivalence(datas, status, coef, ranges)


def restart_grid():
    """[(label, bytes)]: the grid of test_jpeg_cpu.test_restart_intervals plus an interval beyond the MCU count."""
    out = []
    for kw in RESTART_KW:
        for h, w in ((17, 33), (48, 64), (75, 100)):
            for sub in SUBSAMPLINGS:
                out.append(("%dx%d-%s-%r" % (h, w, sub, kw), encode(pixels(h, w, "noise", seed=3), sub, 90, **kw)))
    return out


def quantiser_streams(sub):
    """{K: bytes}: a quality-100 noise image written with one restart interval per MCU row, every quantiser rewritten to K."""
    base = encode(pixels(64, 64, "noise", seed=9), sub, 100, restart_marker_rows=1)
    return {k: _with_quantisers(base, k) for k in list(range(1, 41)) + [64, 128, 255]}


def mutation_files():
    """The files whose scans are mutated: 48 x 64 noise, per sampling class, per MCU row and every 3 MCUs."""
    return [encode(pixels(48, 64, "noise", seed=3), sub, 90, **kw) for sub in SUBSAMPLINGS
            for kw in ({"restart_marker_rows": 1}, {"restart_marker_blocks": 3})]


def mutated(data, file_index, count=200):
    """`count` seeded single-byte mutations of `data` inside its scan (index -> bytes, all of them, accepted or not)."""
    _, scan, cuts = ops.jpeg_scan(data)
    rng = np.random.RandomState(1000 + file_index)
    out = []
    for _ in range(count):
        at = int(rng.randint(scan.scan_begin, cuts[-1]))
        b = bytearray(data)
        b[at] ^= int(rng.randint(1, 256))
        out.append(bytes(b))
    return out


# (file index in mutation_files(), mutation index): three mutations that ds_jpeg_probe accepts and the decoder flags -- what
# tests/test_jpeg_entropy_gpu.py runs through the kernel; test_single_byte_mutations asserts that they are what they claim
FLAGGED_MUTATIONS = ((0, 0), (3, 1), (6, 0))


def test_segment_decoder_equals_the_stream_decoder_on_the_restart_grid():
    items = restart_grid()
    datas = [d for _, d in items]
    assert max(ops.jpeg_scan(d)[2].size for d in datas) > 8            # a file with more than eight segments
    assert any(ops.jpeg_scan(d)[2].size == 1 and ops.jpeg_probe(d).restart_interval > 0 for d in datas)
    assert decode_on_host(datas) == 0
    for d in datas[::7]:                                               # and one image per call
        assert decode_on_host([d]) == 0


@pytest.mark.parametrize("sub", SUBSAMPLINGS)
def test_segment_decoder_applies_the_column_bound(sub):
    streams = quantiser_streams(sub)
    ks = sorted(streams)
    flagged = decode_on_host([streams[k] for k in ks])
    assert 0 < flagged < len(ks)
    assert ops.jpeg_entropy_decode(streams[255], ops.jpeg_probe(streams[255])) is None


def test_single_byte_mutations_inside_the_scan():
    accepted = flagged = 0
    for fi, data in enumerate(mutation_files()):
        batch = [m for m in mutated(data, fi) if ops.jpeg_probe(m) is not None]
        accepted += len(batch)
        flagged += decode_on_host(batch + [data])                      # the intact file behind its damaged copies: still exact
    assert accepted >= 100 * len(mutation_files()) and 0 < flagged < accepted
    files = mutation_files()
    for fi, k in FLAGGED_MUTATIONS:
        m = mutated(files[fi], fi)[k]
        assert ops.jpeg_probe(m) is not None and ops.jpeg_entropy_decode(m, ops.jpeg_probe(m)) is None, (fi, k)


def test_check_jpeg_scan_descs_rejects_what_would_leave_the_buffers():
    datas = [d for _, d in restart_grid()[:6]]
    scan, images, segs, ncoef, _ = tables_with_guards(datas)
    ops.check_jpeg_scan_descs(images, segs, scan.size, ncoef)
    for field, value in (("sampling", 4), ("width", 0), ("coef_offset", 4), ("coef_offset", ncoef), ("first_segment", segs.size),
                         ("segments", 0), ("segments", segs.size + 1), ("reserved", 1)):
        bad = images.copy()
        bad[field][1] = value
        with pytest.raises(ValueError):
            ops.check_jpeg_scan_descs(bad, segs, scan.size, ncoef)
    bad = images.copy()
    bad["coef_offset"][1] = bad["coef_offset"][0]
    with pytest.raises(ValueError, match="share"):
        ops.check_jpeg_scan_descs(bad, segs, scan.size, ncoef)
    for field, value in (("begin", -1), ("end", scan.size + 1), ("mcus", 0), ("first_mcu", 1)):
        bad = segs.copy()
        bad[field][0] = value
        with pytest.raises(ValueError):
            ops.check_jpeg_scan_descs(images, bad, scan.size, ncoef)
    bad = segs.copy()
    bad["mcus"][int(images["segments"][0]) - 1] += 1                   # the last segment of image 0 runs past its MCUs
    with pytest.raises(ValueError, match="sequence"):
        ops.check_jpeg_scan_descs(images, bad, scan.size, ncoef)
    with pytest.raises(ValueError):
        ops.check_jpeg_scan_descs(images[:0], segs, scan.size, ncoef)


def test_switch_is_refused_where_it_cannot_apply():
    from tumblr_emotions_amd.image_model.im_model import load_batch_with_text
    from tumblr_emotions_amd.input_pipeline import DeviceLoader
    with pytest.raises(ValueError, match="jpeg_entropy"):
        load_batch_with_text(None, pipeline="device", jpeg_entropy="device")
    with pytest.raises(ValueError, match="jpeg_entropy"):
        load_batch_with_text(None, pipeline="device", jpeg_decode="device", jpeg_entropy="gpu")
    with pytest.raises(ValueError, match="jpeg_entropy"):
        DeviceLoader(None, jpeg_decode="host", jpeg_entropy="device")
    from tumblr_emotions_amd.training import SyntheticInput
    with pytest.raises(ValueError, match="jpeg_entropy"):
        SyntheticInput()._init_input({"jpeg_entropy": "device", "synthetic": True}, 50, 10, 3, True, "cpu")
    with pytest.raises(ValueError, match="jpeg_entropy"):
        SyntheticInput()._init_input({"jpeg_entropy": "device", "input_pipeline": "device", "synthetic": True}, 50, 10, 3, True, "cpu")
    SyntheticInput()._init_input({"jpeg_entropy": "host", "synthetic": True}, 50, 10, 3, True, "cpu")


def test_eligibility_follows_the_restart_interval():
    from tumblr_emotions_amd.input_pipeline import DEVICE_ENTROPY_MAX_INTERVAL, JpegCoefs, JpegScan, decode_record_jpeg_scan, device_entropy_eligible
    from tumblr_emotions_amd.datasets.tfrecord import encode_example
    a = pixels(75, 100, "noise", seed=3)
    plain, rows = encode(a, 2, 90), encode(a, 2, 90, restart_marker_rows=1)
    wide = pixels(16, 1200, "gradient")                               # 75 MCUs per row at 4:2:0: beyond the constant
    long_rows = encode(wide, 2, 90, restart_marker_rows=1)
    too_long = encode(wide, 2, 90, restart_marker_blocks=76)
    assert DEVICE_ENTROPY_MAX_INTERVAL == 64
    assert not device_entropy_eligible(ops.jpeg_probe(plain)) and device_entropy_eligible(ops.jpeg_probe(rows))
    assert device_entropy_eligible(ops.jpeg_probe(long_rows)) and not device_entropy_eligible(ops.jpeg_probe(too_long))
    assert device_entropy_eligible(ops.jpeg_probe(encode(a, 2, 90, restart_marker_blocks=64)))
    assert not device_entropy_eligible(ops.jpeg_probe(encode(a, 2, 90, restart_marker_blocks=65)))
    rec = lambda d: encode_example({"image/encoded": d, "text": [3, 1, 4], "seq_len": 3, "image/class/label": 2, "post_id": 5, "day": 1})
    got = decode_record_jpeg_scan(rec(rows))
    assert isinstance(got[0], JpegScan) and got[0].data == rows and got[0].cuts.size == 5 and got[2:] == (3, 2, 5, 1)
    assert isinstance(decode_record_jpeg_scan(rec(plain))[0], JpegCoefs)
    bio = io.BytesIO()
    Image.fromarray(a).save(bio, "JPEG", progressive=True)
    assert isinstance(decode_record_jpeg_scan(rec(bio.getvalue()))[0], np.ndarray)
