"""ds_jpeg_entropy_decode_device against the host decoder: for every image of a launch, status 0 exactly when
ds_jpeg_entropy_decode returns DS_OK and then all coefficients equal, guard bands around and between the images' ranges
untouched -- over the restart grid of tests/test_jpeg_restart_cpu.py with the four sampling classes mixed in one batch, a
500 x 375 image, optimised tables, a quality-100 noise image (stuffed bytes, 16-bit codes); flagged images (the column
bound, three recorded mutations) between exact neighbours; and jpeg_entropy='device' end to end: the loader's batches equal
those of jpeg_decode='device' alone and of the host pipeline, bit for bit and in the same order.  Every stream here went
through the same shared lines on the CPU in test_jpeg_restart_cpu.py first."""
import io
import os
import threading

import numpy as np
import pytest
import torch
from PIL import Image

from test_input_pipeline_jpeg_gpu import KEYS, _next
from test_jpeg_cpu import encode, pixels
from test_jpeg_restart_cpu import (FLAGGED_MUTATIONS, PATTERN, check_equivalence, mutated, mutation_files, quantiser_streams,
                                   restart_grid, tables_with_guards)
from tumblr_emotions_amd import ops
from tumblr_emotions_amd.image_model.im_model import load_batch_with_text

pytestmark = pytest.mark.gpu


def decode_on_device(datas):
    """One launch over `datas`; the equivalence contract and the guard bands; returns (flagged images, status)."""
    scan, images, segs, ncoef, ranges = tables_with_guards(datas)
    coef = torch.full((ncoef,), PATTERN, dtype=torch.int16, device="cuda")
    status = ops.jpeg_entropy_decode_device(torch.from_numpy(scan).cuda(), images, segs, coef)
    torch.cuda.synchronize()
    status = status.cpu().numpy()
    host = np.full(ncoef, PATTERN, np.int16)
    assert np.array_equal(status, ops.jpeg_entropy_decode_segments_host(scan, images, segs, host))      # the same bits, flag for flag
    return check_equivalence(datas, status, coef.cpu().numpy(), ranges), status


def test_kernel_equals_the_host_decoder_on_the_restart_grid():
    datas = [d for _, d in restart_grid()]                     # 72 images, the four sampling classes interleaved
    assert decode_on_device(datas)[0] == 0
    assert decode_on_device(datas[5:6])[0] == 0                # a launch of one image


def test_kernel_equals_the_host_decoder_on_large_optimised_and_dense_streams():
    datas = [encode(pixels(375, 500, "noise", seed=1), 2, 90, restart_marker_rows=1)]          # 24 segments of 32 MCUs
    assert ops.jpeg_scan(datas[0])[2].size == 24
    for sub in (0, 1, 2, "L"):
        for content in ("gradient", "noise"):                  # optimised tables; the transcoder replaces some of them
            datas.append(ops.jpeg_restart_transcode(encode(pixels(75, 100, content), sub, 30, optimize=True), 0))
    dense = encode(pixels(64, 64, "noise", seed=9), 0, 100, restart_marker_rows=1)
    assert b"\xff\x00" in dense[ops.jpeg_scan(dense)[1].scan_begin:]                              # stuffed bytes
    assert any(ops.jpeg_scan(dense)[1].ac[c].counts[15] for c in range(3))                     # 16-bit codes
    datas.append(dense)
    datas.append(ops.jpeg_restart_transcode(encode(pixels(64, 64, "noise", seed=9), 2, 100), 1))       # 16 one-MCU segments
    datas.append(encode(pixels(40, 300, "noise", seed=2), "L", 90, restart_marker_blocks=1))           # 190 segments: lanes of every wave
    flagged, _ = decode_on_device(datas)
    assert flagged == 0


def test_flagged_images_leave_their_neighbours_exact():
    files = mutation_files()
    datas = [files[0], quantiser_streams(2)[255], files[3]]
    for fi, k in FLAGGED_MUTATIONS:
        datas += [mutated(files[fi], fi)[k], files[fi]]
    flagged, status = decode_on_device(datas)
    assert flagged == 4 and status[1] != 0 and status[0] == 0 and status[2] == 0
    streams = quantiser_streams(0)
    ks = sorted(streams)
    flagged, status = decode_on_device([streams[k] for k in ks])               # the bound is where the host puts it
    assert 0 < flagged < len(ks) and status[0] == 0 and status[-1] != 0


def test_bad_arguments_are_errors_before_the_launch():
    datas = [d for _, d in restart_grid()[:3]]
    scan, images, segs, ncoef, _ = tables_with_guards(datas)
    coef = torch.zeros(ncoef, dtype=torch.int16, device="cuda")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.jpeg_entropy_decode_device(torch.from_numpy(scan), images, segs, coef)
    bad = segs.copy()
    bad["end"][0] = scan.size + 1
    with pytest.raises(ValueError):
        ops.jpeg_entropy_decode_device(torch.from_numpy(scan).cuda(), images, bad, coef)
    bad = images.copy()
    bad["coef_offset"][2] = ncoef
    with pytest.raises(ValueError):
        ops.jpeg_entropy_decode_device(torch.from_numpy(scan).cuda(), bad, segs, coef)
    with pytest.raises(ValueError, match="status"):
        ops.jpeg_entropy_decode_device(torch.from_numpy(scan).cuda(), images, segs, coef,
                                       status=torch.zeros(2, dtype=torch.int32, device="cuda"))


# ---- the loader -----------------------------------------------------------------------------------------------------------------
N, BATCH = 24, 8
PROGRESSIVE, FLAGGED = 7, 13                     # post ids


def _dataset(root):
    """24 records in two shards: restart-marked files (Pillow's and the transcoder's), plain baseline files, one
    progressive file and one restart-marked file the decoder flags (the column bound); returns (Dataset, restart-marked ids)."""
    from tumblr_emotions_amd.datasets.convert_to_dataset import Dataset
    from tumblr_emotions_amd.datasets.tfrecord import encode_example, write_records
    os.makedirs(root, exist_ok=True)
    rng = np.random.RandomState(5)
    sizes = ((75, 100), (64, 48), (33, 17), (120, 90), (16, 16), (50, 75))
    paths, marked = [], set()
    for shard in range(2):
        recs = []
        for i in range(shard * N // 2, (shard + 1) * N // 2):
            h, w = sizes[i % len(sizes)]
            yy, xx = np.mgrid[0:h, 0:w]
            a = (np.stack([yy * 3, xx * 2, yy + xx], -1) + rng.randint(0, 60, (h, w, 3))).astype(np.uint8)
            sub = (0, 1, 2, "L")[i % 4]
            if i == PROGRESSIVE:
                bio = io.BytesIO()
                Image.fromarray(a).save(bio, "JPEG", quality=90, progressive=True)
                data = bio.getvalue()
            elif i == FLAGGED:
                data = quantiser_streams(2)[255]
                assert ops.jpeg_probe(data).restart_interval > 0 and ops.jpeg_entropy_decode(data, ops.jpeg_probe(data)) is None
            elif i % 3 == 0:
                data = encode(a, sub, (60, 90, 100)[i % 3], restart_marker_rows=1)
                marked.add(i)
            elif i % 3 == 1:
                data = ops.jpeg_restart_transcode(encode(a, sub, 85, optimize=True), 2)
                marked.add(i)
            else:
                data = encode(a, sub, 90)
            n = 1 + i % 9
            recs.append(encode_example({"image/encoded": data, "image/format": b"jpg", "image/class/label": i % 3,
                                        "text": [int(t) for t in rng.randint(0, 100, n)], "seq_len": n, "post_id": i, "day": i % 7}))
        paths.append(os.path.join(root, "tumblr_train_%05d-of-00002.tfrecord" % shard))
        write_records(paths[-1], recs)
    return Dataset(paths, N, 3, {0: "a", 1: "b", 2: "c"}), marked


@pytest.mark.parametrize("is_training", (False, True))
def test_device_entropy_stream_equals_the_other_two(tmp_path, is_training):
    ds, marked = _dataset(str(tmp_path / "d"))
    kw = dict(batch_size=BATCH, shuffle=is_training, height=224, width=224, is_training=is_training, seed=4, max_token_id=100,
              num_classes=3)
    before = threading.active_count()
    steps = 2 * N // BATCH                                       # two passes: the three staging sets are used twice
    host = load_batch_with_text(ds, pipeline="host", **kw)
    with load_batch_with_text(ds, pipeline="device", workers=4, jpeg_decode="device", jpeg_entropy="device", **kw) as dev, \
            load_batch_with_text(ds, pipeline="device", workers=4, jpeg_decode="device", **kw) as parent:
        assert dev.jpeg_entropy == "device" and parent.jpeg_entropy == "host"
        on_device = 0
        for step in range(steps):
            a, b, c = _next(dev), _next(parent), next(host)
            assert a is not None and b is not None
            for k in KEYS:
                assert a[k].dtype == b[k].dtype == c[k].dtype, (step, k)
                assert torch.equal(a[k], b[k]) and torch.equal(a[k], c[k]), (step, k)
            on_device += sum(int(p) in marked for p in a["post_ids"].tolist())
            assert dev.jpeg_fallbacks == parent.jpeg_fallbacks and dev.jpeg_device_entropy == on_device
            assert parent.jpeg_device_entropy == 0
        assert dev.jpeg_fallbacks == 4 and on_device == 2 * len(marked) > 0        # (progressive + flagged) x two passes
    host.close()
    torch.cuda.synchronize()
    assert threading.active_count() == before
