"""jpeg_decode='device' end to end: the batch stream of the device pipeline with the compiled Huffman decode and
ds_jpeg_reconstruct equals, tensor for tensor and bit for bit, the stream of the same pipeline decoding with PIL -- eval
chain and is_training=True, shuffle on and off, 1 and 8 workers, two passes -- and jpeg_fallbacks counts the progressive
records consumed.  The dataset (40 records, mixed sizes and subsamplings, two progressive files) is written to tmp_path from
seeds.  Every wait on the loader has its own time limit."""
import io
import os
import re
import threading

import numpy as np
import pytest
import torch
from PIL import Image

from tumblr_emotions_amd.image_model.im_model import load_batch_with_text
from tumblr_emotions_amd.input_pipeline import DeviceLoader

pytestmark = pytest.mark.gpu
KEYS = ("images", "texts", "seq_lens", "labels", "post_ids", "days")
N, BATCH = 40, 8
PROGRESSIVE = (7, 23)                       # post ids of the two progressive files
STEP_LIMIT = 60.0                           # seconds for one batch of 8 small images (it takes milliseconds)


def _dataset(root):
    from tumblr_emotions_amd.datasets.convert_to_dataset import Dataset
    from tumblr_emotions_amd.datasets.tfrecord import encode_example, write_records
    os.makedirs(root, exist_ok=True)
    rng = np.random.RandomState(11)
    sizes = ((75, 100), (64, 48), (33, 17), (120, 90), (16, 16), (50, 75))
    paths = []
    for shard in range(2):
        recs = []
        for i in range(shard * N // 2, (shard + 1) * N // 2):
            h, w = sizes[i % len(sizes)]
            yy, xx = np.mgrid[0:h, 0:w]
            a = (np.stack([yy * 3, xx * 2, yy + xx], -1) + rng.randint(0, 60, (h, w, 3))).astype(np.uint8)
            bio = io.BytesIO()
            if i % 5 == 4:
                Image.fromarray(a).convert("L").save(bio, "JPEG", quality=85)
            else:
                Image.fromarray(a).save(bio, "JPEG", quality=(60, 90, 100)[i % 3], subsampling=i % 3, progressive=i in PROGRESSIVE)
            n = 1 + i % 9
            recs.append(encode_example({"image/encoded": bio.getvalue(), "image/format": b"jpg", "image/class/label": i % 3,
                                        "text": [int(t) for t in rng.randint(0, 100, n)], "seq_len": n, "post_id": i, "day": i % 7}))
        paths.append(os.path.join(root, "tumblr_train_%05d-of-00002.tfrecord" % shard))
        write_records(paths[-1], recs)
    return Dataset(paths, N, 3, {0: "a", 1: "b", 2: "c"})


def _next(loader):
    """next(loader) under a time limit of its own."""
    box = []

    def step():
        try:
            box.append((next(loader, None), None))
        except BaseException as e:             # noqa: BLE001 -- handed to the caller, raised there
            box.append((None, e))

    t = threading.Thread(target=step, daemon=True)
    t.start()
    t.join(STEP_LIMIT)
    assert not t.is_alive(), "the loader did not deliver a batch within %.0f s" % STEP_LIMIT
    if box[0][1] is not None:
        raise box[0][1]
    return box[0][0]


@pytest.mark.parametrize("workers", (1, 8))
@pytest.mark.parametrize("shuffle", (False, True))
@pytest.mark.parametrize("is_training", (False, True))
def test_device_jpeg_stream_equals_the_pil_stream(tmp_path, is_training, shuffle, workers):
    ds = _dataset(str(tmp_path / "d"))
    kw = dict(batch_size=BATCH, shuffle=shuffle, height=224, width=224, is_training=is_training, seed=4, pipeline="device",
              workers=workers, max_token_id=100, num_classes=3)
    before = threading.active_count()
    steps = 2 * N // BATCH                                       # two passes
    with load_batch_with_text(ds, jpeg_decode="device", **kw) as dev, load_batch_with_text(ds, jpeg_decode="host", **kw) as host:
        assert isinstance(dev, DeviceLoader) and dev.jpeg_decode == "device" and host.jpeg_decode == "host"
        progressive = 0
        for step in range(steps):
            a, b = _next(dev), _next(host)
            assert a is not None and b is not None
            for k in KEYS:
                assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), (step, k)
            progressive += sum(int(p) in PROGRESSIVE for p in a["post_ids"].tolist())
            assert dev.jpeg_fallbacks == progressive and host.jpeg_fallbacks == 0
        assert progressive == 4
    torch.cuda.synchronize()
    assert threading.active_count() == before


def test_a_corrupt_file_raises_what_it_raises_today(tmp_path):
    from tumblr_emotions_amd.datasets.convert_to_dataset import Dataset
    from tumblr_emotions_amd.datasets.tfrecord import encode_example, read_records, write_records
    ds = _dataset(str(tmp_path / "d"))
    recs = [bytes(r) for r in read_records(ds.data_sources[0])]
    bio = io.BytesIO()
    Image.fromarray(np.zeros((40, 40, 3), np.uint8)).save(bio, "JPEG")
    recs[3] = encode_example({"image/encoded": bio.getvalue()[:200], "image/class/label": 0, "text": [1], "seq_len": 1,
                              "post_id": 99, "day": 0})
    path = str(tmp_path / "bad.tfrecord")
    write_records(path, recs)
    bad = Dataset([path], len(recs), 3, {0: "a", 1: "b", 2: "c"})
    errors = []
    for mode in ("host", "device"):
        with load_batch_with_text(bad, batch_size=4, shuffle=False, height=64, width=64, pipeline="device", workers=2,
                                  jpeg_decode=mode) as it:
            with pytest.raises(OSError) as e:
                _next(it)
            errors.append((type(e.value), re.sub(r"0x[0-9a-fA-F]+", "0x", str(e.value))))      # (object addresses differ)
    assert errors[0] == errors[1]
