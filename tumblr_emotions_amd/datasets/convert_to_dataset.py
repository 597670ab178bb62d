"""`get_split_with_text` without TensorFlow (datasets/convert_to_dataset.py:117-198): describes a split
of the Tumblr dataset (sharded TFRecords of image + token ids) and iterates its decoded examples."""
import glob
import io
import os

import numpy as np

from . import dataset_utils
from .tfrecord import decode_example, read_records

_FILE_PATTERN = 'tumblr_%s_*.tfrecord'                  # convert_to_dataset.py:29
_TRAIN_VALID_FILENAME = 'train_valid_split.txt'         # :32
_POST_SIZE = 50                                         # :34
_NUM_SHARDS = 5                                         # datasets/convert_images_tfrecords.py


def dataset_filename(dataset_dir, subdir, split_name, shard_id, num_shards=_NUM_SHARDS):
    """Shard naming of convert_images_tfrecords.py:110-113."""
    return os.path.join(dataset_dir, subdir, 'tumblr_%s_%05d-of-%05d.tfrecord' % (split_name, shard_id, num_shards))


class Dataset:
    """The fields of slim.dataset.Dataset the trainers read, plus an example iterator."""

    def __init__(self, data_sources, num_samples, num_classes, labels_to_names):
        self.data_sources, self.num_samples = data_sources, num_samples
        self.num_classes, self.labels_to_names = num_classes, labels_to_names

    def examples(self, verify_crc=False, decode_image=None):
        """Yields dicts: image (uint8 HxWx3), text (int64[50]), seq_len, label, post_id, day
        (the items_to_handlers of convert_to_dataset.py:163-170).  decode_image(index) -> bool lets a
        data-parallel reader skip the JPEG decode of records that belong to other ranks (image = None)."""
        from PIL import Image
        idx = -1
        for path in self.data_sources:
            for rec in read_records(path, verify=verify_crc):
                idx += 1
                ex = decode_example(rec)
                img = None
                if decode_image is None or decode_image(idx):
                    img = np.asarray(Image.open(io.BytesIO(ex['image/encoded'][0])).convert('RGB'))
                text = np.zeros(_POST_SIZE, np.int64)
                t = ex.get('text', [])
                text[:len(t)] = t
                yield dict(image=img, text=text, seq_len=int(ex.get('seq_len', [0])[0]),
                           label=int(ex.get('image/class/label', [0])[0]), post_id=int(ex.get('post_id', [0])[0]),
                           day=int(ex.get('day', [0])[0]))


def get_split_with_text(split_name, dataset_dir, photos_subdir='photos', tfrecords_subdir='tfrecords',
                        file_pattern=None, reader=None):
    pattern = os.path.join(dataset_dir, tfrecords_subdir, (file_pattern or _FILE_PATTERN) % split_name)
    labels_to_names = None
    if dataset_utils.has_labels(dataset_dir, photos_subdir):
        labels_to_names = dataset_utils.read_label_file(dataset_dir, photos_subdir)
    with open(os.path.join(dataset_dir, photos_subdir, _TRAIN_VALID_FILENAME), 'rb') as f:
        lines = [l for l in f.read().decode().split('\n') if l]
    sizes = {}
    for line in lines:
        i = line.index(':')
        sizes[line[:i]] = int(line[i + 1:])
    return Dataset(sorted(glob.glob(pattern)), sizes[split_name], len(labels_to_names), labels_to_names)


def add_restart_markers(dataset_dir, tfrecords_subdir='tfrecords', out_subdir='tfrecords_rst', interval_mcus=0):
    """Rewrite every shard of dataset_dir/tfrecords_subdir under the same file name into dataset_dir/out_subdir with
    'image/encoded' re-encoded LOSSLESSLY with a restart interval of interval_mcus MCUs (0 = one MCU row): the Huffman data
    of such a stream can be decoded segment by segment, which load_batch_with_text(jpeg_entropy='device') does on the GPU.
    The coefficients, and so the pixels, do not change (ds_jpeg_restart_transcode).  A stream outside the compiled
    decoder's supported set (progressive, CMYK, ...) keeps its bytes; every other feature and the record order are
    unchanged.  get_split_with_text(..., tfrecords_subdir=out_subdir) reads the result.  Returns (transcoded, kept)."""
    from .. import ops
    from .tfrecord import encode_example, write_records
    src, dst = os.path.join(dataset_dir, tfrecords_subdir), os.path.join(dataset_dir, out_subdir)
    if os.path.abspath(src) == os.path.abspath(dst):
        raise ValueError("add_restart_markers: out_subdir must differ from tfrecords_subdir")
    os.makedirs(dst, exist_ok=True)
    transcoded = kept = 0
    for path in sorted(glob.glob(os.path.join(src, '*.tfrecord'))):
        records = []
        for rec in read_records(path):
            rec = bytes(rec)
            ex = decode_example(rec)
            images = ex.get('image/encoded', [])
            new = ops.jpeg_restart_transcode(images[0], interval_mcus) if images else None
            if new is None:
                kept += 1
                records.append(rec)
                continue
            transcoded += 1
            ex['image/encoded'] = [new] + images[1:]
            records.append(encode_example(ex))
        write_records(os.path.join(dst, os.path.basename(path)), records)
    return transcoded, kept
