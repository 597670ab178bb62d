"""Device input pipeline: the batches of `image_model.im_model.load_batch_with_text`, bit for bit and in the same order,
with the preprocessing on the GPU (ds_preprocess_eval; ds_preprocess_train with is_training=True), the JPEG decode on a bounded pool of worker threads, and
the upload + preprocessing of the next batches overlapped with the training step.

    records (main feeder thread, file order)         raw TFRecord payloads of THIS rank only
      -> OrderedPool (<= 16 daemon threads)          decode_example + PIL decode + central crop   (GIL released in PIL / NumPy)
      -> feeder, in submission order                 checks, ragged packing into a pinned staging set, descriptor table
      -> copy stream                                 non_blocking uploads, ds_preprocess_eval behind them, an event
      -> DeviceLoader.__next__                       the consumer's stream waits for the event and takes the tensors

The crop offsets / extents and the resize scales are computed with the very expressions of
preprocessing/inception_preprocessing.py (Python doubles, then np.float32), so the kernel repeats no double arithmetic.
With is_training=True a worker draws the record's augmentation parameters after the decode (the image size is known only
then) from record_rng(seed, pass, global record index) -- the host generator's stream, so the batches stay equal whatever
the worker count -- and slices the sampled crop instead of the central one; the feeder fills ds_preprocess_train_desc records.
Source shuffling, the in-batch permutation and the ragged tail draw from one RandomState in the host generator's
sequence.  Staging sets are filled by the feeder (not by the workers: an image's offset in the ragged buffer is known
only once every earlier image of the batch has been decoded) and are reused only after the event of their last upload
has completed.

jpeg_decode='device' (opt-in) moves the decode itself off PIL: a worker makes ONE call into compiled host code per record
(ds_jpeg_record_decode: the tf.Example parse, the JPEG marker parse and the Huffman decode, the GIL released throughout)
and returns quantised DCT coefficients instead of pixels; the image size comes from the header, so the central crop -- or,
with is_training=True, the draws of sample_train_params -- are made before any pixel exists.  The feeder packs coefficients
and ds_jpeg_desc records into the staging set, and ds_jpeg_reconstruct (inverse DCT, upsampling, colour conversion, crop)
writes the ragged byte buffer on the copy stream in front of the unchanged preprocessing kernel.  A stream outside the
decoder's supported set (progressive, CMYK, ...) takes the PIL path for that image alone -- its pixels are uploaded into
their slot of the same buffer, a corrupt file raises what it raises today -- and is counted in DeviceLoader.jpeg_fallbacks.

jpeg_entropy='device' (opt-in, with jpeg_decode='device' only) moves the Huffman decode of restart-segmented streams to the
GPU as well: for a supported stream whose restart interval is short enough (device_entropy_eligible) the worker only parses
markers (ds_jpeg_record_scan) and hands over a JpegScan -- the encoded bytes, the header's tables and the positions of the
restart markers; the feeder packs the entropy-coded bytes and two small tables into pinned staging and
ds_jpeg_entropy_decode_device writes the coefficients where ds_jpeg_reconstruct reads them, so neither a coefficient buffer
nor its upload exists on the host.  The feeder reads the per-image status words back (it blocks on that event; the consumer
does not, the feeder runs `prefetch` batches ahead) and decodes a flagged image with PIL from the bytes it still holds: a
fallback like any other.  Every other image of the batch goes the way it goes with jpeg_entropy='host'.
datasets.convert_to_dataset.add_restart_markers gives a converted dataset one restart interval per MCU row, losslessly.

cache='device' (opt-in, with an explicit cache_bytes) keeps the decoded uint8 pixels of every record in one arena of device
memory: a record -- (index of its file in dataset.data_sources, index in the file) -- is decoded once, the way the loader is
configured, and its pixels are written INTO THE ARENA (an H2D copy for the PIL path; ds_jpeg_reconstruct writes there
itself): the central crop, or with is_training=True the whole image, whose crop changes from pass to pass while the pixels
do not.  Every image of a batch, hit or miss, is then moved into the ragged buffer by ONE ds_ragged_gather launch on the copy
stream, and the preprocessing kernel runs as ever.  A record is resident from the moment the feeder takes it off the decode
queue (its arena offset is reserved there; the write is enqueued with its batch, ahead of every gather that reads it).  The
record stream opens a file only when it does not know its size yet or a record of this rank in it is not resident, so a fully
cached pass opens nothing and submits nothing to the pool; a pass starts only when the one before it has been consumed, so what
is resident is known.  Nothing is evicted: once an image finds no room, nothing more is inserted, and such records are decoded
on every pass into the staging set's spill buffer, which the same gather reads.

Whatever the switches, a batch ends in the same two things -- the ragged byte buffer, laid out as pack_ragged lays it out, and
the preprocessing descriptor table -- and is made by the same three steps.  _next_item turns a record of the stream into an
_Item: what still has to be written for the image (a decoded array, JpegCoefs, JpegScan; nothing for a hit of the cache), the
region that produces and the window of it that goes to the ragged buffer.  pack_batch, host only, lays the items out and
returns a BatchPlan: the H2D copies, the ds_jpeg_desc rows grouped by the buffer they write (the ragged buffer; with the cache
the arena and the spill buffer, followed by the gather), the coefficient uploads and the scan tables.  _run_plan issues the
plan on the copy stream -- copies, entropy launch or coefficient upload, flagged_fallback (host only as well: it amends the
plan for the images the Huffman kernel flagged), ds_jpeg_reconstruct once per buffer, the gather -- in front of the
preprocessing kernel.  tests/test_input_batch_plan_cpu.py executes the same plans with the kernels' host statements.
"""
import collections
import functools
import io
import queue
import threading
import weakref

import numpy as np

MAX_WORKERS = 16
CENTRAL_FRACTION = 0.875              # preprocess_for_eval's default, the only value the reference uses
_FIELDS = (("seq_lens", "seq_len"), ("labels", "label"), ("post_ids", "post_id"), ("days", "day"))


# ---- geometry: the host half of preprocess_for_eval -------------------------------------------------------------------------
def crop_box(h, w, central_fraction=CENTRAL_FRACTION):
    """(y0, x0, crop_h, crop_w) of central_crop for an h x w image -- its own expressions, in Python doubles."""
    if not central_fraction:
        return 0, 0, h, w
    h0 = int((h - h * central_fraction) / 2)
    w0 = int((w - w * central_fraction) / 2)
    return h0, w0, h - 2 * h0, w - 2 * w0


def resize_scale(n_in, n_out):
    """The fp32 scale of resize_bilinear's axis(): np.float32(n_in / n_out), the division in double."""
    return np.float32(n_in / n_out)


def clamp_workers(workers):
    """1 <= workers <= 16, whatever the machine has (never sized from os.cpu_count())."""
    return max(1, min(int(workers), MAX_WORKERS))


def _round_up(n, m):
    return -(-n // m) * m


def _check_image(im, what):
    if im.ndim != 3 or im.shape[2] != 3 or im.dtype != np.uint8 or im.shape[0] < 1 or im.shape[1] < 1:
        raise ValueError("%s: images must be non-empty uint8 [h, w, 3] arrays" % what)


def _crop(h, w, train_key=None, whole=False):
    """(box, TrainParams or None) of an h x w image: the whole image, the central crop, or the crop sample_train_params
    draws from record_rng(*train_key)."""
    if whole:
        return (0, 0, h, w), None
    if train_key is None:
        return crop_box(h, w), None
    from .preprocessing.inception_preprocessing import record_rng, sample_train_params
    p = sample_train_params(h, w, record_rng(*train_key))
    return (p.y0, p.x0, p.crop_h, p.crop_w), p


def _desc_record(off, h, w, out_h, out_w, p=None):
    """One ds_preprocess_desc record (p None) or ds_preprocess_train_desc record of a crop of h x w pixels at byte `off`."""
    geom = (off, h, w, resize_scale(h, out_h), resize_scale(w, out_w))
    if p is None:
        return geom
    from ._lib import DS_PREPROCESS_FLIP, DS_PREPROCESS_SATURATION_FIRST
    flags = (DS_PREPROCESS_FLIP if p.flip else 0) | (DS_PREPROCESS_SATURATION_FIRST if p.saturation_first else 0)
    return geom + (p.delta, p.factor, flags, 0)


def pack_ragged(images, out_h, out_w, out=None, desc=None, align=4, params=None):
    """Lay cropped uint8 HWC images back to back (each start rounded up to `align` bytes) and describe them.
    images: list of [h, w, 3] uint8 arrays; out: uint8 buffer to fill (a new one when None; ValueError when too small);
    desc: descriptor array to fill (first len(images) records); params: one TrainParams per image (the images are their
    sampled crops) -- the descriptors are then ds_preprocess_train_desc records.  Returns (buffer, descriptors, bytes used)."""
    from .ops import preprocess_desc_dtype, preprocess_train_desc_dtype
    n = len(images)
    if params is not None and len(params) != n:
        raise ValueError("pack_ragged: one parameter set per image")
    if desc is None:
        desc = np.zeros(n, preprocess_desc_dtype() if params is None else preprocess_train_desc_dtype())
    offsets, pos = [], 0
    for im in images:
        _check_image(im, "pack_ragged")
        offsets.append(pos)
        pos = _round_up(pos + im.size, align)
    if out is None:
        out = np.zeros(max(pos, align), np.uint8)
    if out.size < pos:
        raise ValueError("pack_ragged: %d bytes do not fit a buffer of %d" % (pos, out.size))
    for i, (im, off) in enumerate(zip(images, offsets)):
        out[off:off + im.size].reshape(im.shape)[...] = im
        p = None if params is None else params[i]
        if p is not None and (p.crop_h, p.crop_w) != im.shape[:2]:
            raise ValueError("pack_ragged: image %d is not the crop its parameters describe" % i)
        desc[i] = _desc_record(off, im.shape[0], im.shape[1], out_h, out_w, p)
    return out, desc[:n], pos


# ---- decode pool ------------------------------------------------------------------------------------------------------------
class _Slot:
    __slots__ = ("done", "value", "error")

    def __init__(self):
        self.done, self.value, self.error = threading.Event(), None, None

    def result(self):
        self.done.wait()
        if self.error is not None:
            raise self.error
        return self.value


def _pool_worker(tasks):
    while True:
        item = tasks.get()
        if item is None:
            return
        slot, fn, args = item
        try:
            slot.value = fn(*args)
        except BaseException as e:          # handed to the consumer, raised at this item's position in the order
            slot.error = e
        slot.done.set()


class OrderedPool:
    """At most 16 daemon threads; submit() returns a slot whose result() blocks -- callers consume slots in submission
    order, so a slow early item delays but never reorders the stream.  close() joins every thread."""

    def __init__(self, workers):
        self.workers = clamp_workers(workers)
        self._tasks = queue.SimpleQueue()
        self._threads = [threading.Thread(target=_pool_worker, args=(self._tasks,), daemon=True,
                                          name="ds-input-decode-%d" % i) for i in range(self.workers)]
        for t in self._threads:
            t.start()

    def submit(self, fn, *args):
        slot = _Slot()
        self._tasks.put((slot, fn, args))
        return slot

    def close(self):
        try:                                   # queued items nobody will consume any more are dropped, not decoded
            while True:
                self._tasks.get_nowait()
        except queue.Empty:
            pass
        for _ in self._threads:
            self._tasks.put(None)
        for t in self._threads:
            t.join()
        self._threads = []


def decode_record(rec, train_key=None, whole=False, *, decode_image=True):
    """One TFRecord payload -> (cropped uint8 image or None, text int64[50], seq_len, label, post_id, day): the work of
    Dataset.examples for one record plus central_crop (only the cropped region is ever uploaded).  train_key = (seed, pass,
    global record index): the crop is the one sample_train_params draws from record_rng(*train_key), and the first item
    is (crop, TrainParams).  whole (cache='device' at train time): the uncropped image, nothing drawn."""
    from .datasets.convert_to_dataset import _POST_SIZE
    from .datasets.tfrecord import decode_example
    ex = decode_example(rec)
    img = None
    if decode_image:
        img = decode_pixels(ex['image/encoded'][0], train_key, whole)
    text = np.zeros(_POST_SIZE, np.int64)
    t = ex.get('text', [])
    text[:len(t)] = t
    return (img, text, int(ex.get('seq_len', [0])[0]), int(ex.get('image/class/label', [0])[0]),
            int(ex.get('post_id', [0])[0]), int(ex.get('day', [0])[0]))


def decode_pixels(data, train_key=None, whole=False):
    """The PIL decode of one encoded image and its crop: the central one, or (crop, TrainParams) for train_key, or -- whole
    -- no crop at all."""
    from PIL import Image
    img = np.asarray(Image.open(io.BytesIO(data)).convert('RGB'))
    (y0, x0, ch, cw), p = _crop(img.shape[0], img.shape[1], train_key, whole)
    crop = np.ascontiguousarray(img[y0:y0 + ch, x0:x0 + cw])
    return crop if p is None else (crop, p)


# ---- jpeg_decode='device': coefficients instead of pixels ----------------------------------------------------------------------
class JpegCoefs:
    """What a worker hands the feeder for an image the device reconstructs: quantised coefficients (int16, the layout of
    ds_jpeg_entropy_decode), the header's geometry and tables, the crop box and, at train time, the TrainParams."""
    __slots__ = ("coef", "height", "width", "sampling", "quant", "box", "params")

    def __init__(self, coef, height, width, sampling, quant, box, params=None):
        self.coef, self.height, self.width, self.sampling, self.quant = coef, height, width, sampling, quant
        self.box, self.params = box, params


_worker = threading.local()

# A stream takes the device entropy path when 0 < restart interval <= max(MCUs per row, this): a lane decodes a segment
# serially, so long segments leave most of a workgroup idle.  The value is a guess that nobody has measured.
DEVICE_ENTROPY_MAX_INTERVAL = 64


def device_entropy_eligible(info):
    """The stream of this _lib.JpegInfo is decoded by ds_jpeg_entropy_decode_device under jpeg_entropy='device'."""
    from . import ops
    mw, _ = ops.jpeg_mcus(int(info.height), int(info.width), int(info.sampling))
    return 0 < info.restart_interval <= max(mw, DEVICE_ENTROPY_MAX_INTERVAL)


class JpegScan:
    """What a worker hands the feeder for an image whose Huffman decode runs on the device: the encoded bytes, the header
    (ds_jpeg_info), the scan's tables and cut positions (ds_jpeg_scan), the crop box and, at train time, the TrainParams
    and the key they were drawn from (a flagged image is decoded by decode_pixels(data, train_key))."""
    __slots__ = ("data", "info", "scan", "cuts", "height", "width", "sampling", "quant", "box", "params", "train_key", "coef_count")

    def __init__(self, data, info, scan, cuts, like, train_key):
        self.data, self.info, self.scan, self.cuts, self.train_key = data, info, scan, cuts, train_key
        self.height, self.width, self.sampling, self.quant = like.height, like.width, like.sampling, like.quant
        self.box, self.params, self.coef_count = like.box, like.params, int(info.coef_count)


def decode_jpeg_bytes(data, train_key=None):
    """One encoded image -> JpegCoefs when the compiled decoder supports the stream, else what decode_pixels returns (the
    PIL path; it raises what PIL raises)."""
    from . import ops
    info = ops.jpeg_probe(data)
    coef = ops.jpeg_entropy_decode(data, info) if info is not None else None
    if coef is None:
        return decode_pixels(data, train_key)
    return _coefs(coef, info, train_key)


def _coefs(coef, info, train_key, whole=False):
    from . import ops
    h, w = int(info.height), int(info.width)
    box, p = _crop(h, w, train_key, whole)
    return JpegCoefs(coef, h, w, int(info.sampling), ops.jpeg_quant(info), box, p)


def decode_record_jpeg(rec, train_key=None, whole=False):
    """decode_record with the compiled path: one ds_jpeg_record_decode call (payload parse + probe + Huffman decode, no GIL);
    the first item is a JpegCoefs, or -- for a stream outside the supported set -- exactly decode_record's.  A payload the
    compiled reader does not take goes through decode_record whole."""
    from . import _lib, ops
    rec = bytes(rec)
    size = max(getattr(_worker, "size", 0), 1 << 16)
    buf = np.empty(size, np.int16)          # handed over to the feeder with the result: a fresh one per record
    r = ops.jpeg_record_decode(rec, buf)
    if r is not None and r[0] == _lib.DS_JPEG_MORE:
        _worker.size = size = int(r[1].coef_count)
        buf = np.empty(size, np.int16)
        r = ops.jpeg_record_decode(rec, buf)
    if r is None:
        return decode_record(rec, train_key, whole)
    status, info, (off, length, text, seq_len, label, post_id, day) = r
    if status == 0:
        img = _coefs(buf[:int(info.coef_count)], info, train_key, whole)
    else:
        img = decode_pixels(rec[off:off + length], train_key, whole)
    return img, text, int(seq_len), int(label), int(post_id), int(day)


def decode_record_jpeg_scan(rec, train_key=None, whole=False):
    """decode_record_jpeg under jpeg_entropy='device': one ds_jpeg_record_scan call (payload parse + marker parse, nothing
    decoded, no GIL); the first item is a JpegScan for an eligible stream, and exactly decode_record_jpeg's otherwise."""
    from . import _lib, ops
    rec = bytes(rec)
    cuts = np.empty(max(getattr(_worker, "cuts", 0), 256), np.int64)      # handed over with the result: a fresh one per record
    r = ops.jpeg_record_scan(rec, cuts)
    if r is not None and r[0] == _lib.DS_JPEG_MORE and device_entropy_eligible(r[1]):
        _worker.cuts = int(r[2].cut_count)
        cuts = np.empty(_worker.cuts, np.int64)
        r = ops.jpeg_record_scan(rec, cuts)
    if r is None or r[0] != 0 or not device_entropy_eligible(r[1]):
        return decode_record_jpeg(rec, train_key, whole)
    _, info, scan, (off, length, text, seq_len, label, post_id, day) = r
    img = JpegScan(rec[off:off + length], info, scan, cuts[:int(scan.cut_count)], _coefs(None, info, train_key, whole), train_key)
    return img, text, int(seq_len), int(label), int(post_id), int(day)


# ---- configuration and staging ------------------------------------------------------------------------------------------------
# What the feeder and its staging sets are built from, made once by DeviceLoader.__init__.  train, jpeg, entropy and
# cache_bytes are normalised there: all off with decode_images=False, entropy only with jpeg, cache_bytes None without the cache.
_Config = collections.namedtuple(
    "_Config", "batch_size height width device decode_images train jpeg entropy cache_bytes shuffle rank world seed loop "
               "max_token_id num_classes prefetch inflight",
    defaults=(True, False, False, False, None, False, 0, 1, 0, True, None, None, 2, 256))

# What the feeder hands DeviceLoader.__next__ per batch, and the cache's share of it (None without the cache).
_Batch = collections.namedtuple("_Batch", "out event stream fallbacks on_device stats")
_CacheStats = collections.namedtuple("_CacheStats", "hits misses spilled records bytes_used")


class _Staging:
    """One pinned staging set: ragged image bytes + descriptor table + the int64 fields, with the device byte buffer and
    descriptor table they are uploaded into and the event of the last upload."""

    def __init__(self, cfg, post_size):
        import torch
        from . import ops
        batch_size, device = cfg.batch_size, cfg.device
        preprocess_desc_dtype = ops.preprocess_train_desc_dtype if cfg.train else ops.preprocess_desc_dtype
        cuda = device.type == "cuda"
        self.torch, self.device, self.cuda = torch, device, cuda
        self.event = None
        self.ints = self._host(batch_size * (post_size + len(_FIELDS)), torch.int64)
        self.desc = self._host(batch_size * preprocess_desc_dtype().itemsize, torch.uint8)
        self.desc_np = self.desc.numpy().view(preprocess_desc_dtype())
        self.desc_dev = torch.empty(self.desc.numel(), dtype=torch.uint8, device=device) if cuda else None
        self.bytes = self.bytes_dev = None
        self.reserve(1 << 20)
        self.coef = self.coef_dev = self.scratch_dev = None
        if cfg.jpeg:              # jpeg_decode='device': coefficients, their descriptors, the planes of ds_jpeg_reconstruct
            self.jdesc = self._host(batch_size * ops.jpeg_desc_dtype().itemsize, torch.uint8)
            self.jdesc_np = self.jdesc.numpy().view(ops.jpeg_desc_dtype())
            self.jdesc_dev = torch.empty(self.jdesc.numel(), dtype=torch.uint8, device=device) if cuda else None
            self.reserve_coef(1 << 20)
        self.scan = self.scan_dev = self.segs = self.segs_np = self.segs_dev = None
        if cfg.entropy:           # jpeg_entropy='device': entropy-coded bytes, the two tables, the status words
            self.sdesc = self._host(batch_size * ops.jpeg_scan_desc_dtype().itemsize, torch.uint8)
            self.sdesc_np = self.sdesc.numpy().view(ops.jpeg_scan_desc_dtype())
            self.status = self._host(batch_size, torch.int32)
            if cuda:
                self.sdesc_dev = torch.empty(self.sdesc.numel(), dtype=torch.uint8, device=device)
                self.status_dev = torch.empty(batch_size, dtype=torch.int32, device=device)
            self.reserve_scan(1 << 20, 1 << 12)
        self.spill_dev = None
        if cfg.cache_bytes:       # cache='device': the ds_ragged_gather table; the spill buffer appears with the first spilled image
            self.gdesc = self._host(batch_size * ops.gather_desc_dtype().itemsize, torch.uint8)
            self.gdesc_np = self.gdesc.numpy().view(ops.gather_desc_dtype())
            self.gdesc_dev = torch.empty(self.gdesc.numel(), dtype=torch.uint8, device=device)

    def _host(self, n, dtype):
        return self.torch.empty(n, dtype=dtype, pin_memory=self.cuda)

    def reserve(self, nbytes):
        if self.bytes is None or self.bytes.numel() < nbytes:
            cap = _round_up(int(nbytes * 1.25), 4096)
            self.bytes = self._host(cap, self.torch.uint8)
            self.bytes_dev = self.torch.empty(cap, dtype=self.torch.uint8, device=self.device) if self.cuda else None

    def reserve_coef(self, n):
        if self.coef is None or self.coef.numel() < n:
            cap = _round_up(int(n * 1.25), 4096)
            self.coef = self._host(cap, self.torch.int16)
            if self.cuda:
                self.coef_dev = self.torch.empty(cap, dtype=self.torch.int16, device=self.device)
                self.scratch_dev = self.torch.empty(cap, dtype=self.torch.uint8, device=self.device)

    def reserve_spill(self, nbytes):
        if nbytes and (self.spill_dev is None or self.spill_dev.numel() < nbytes):
            cap = _round_up(int(nbytes * 1.25), 4096)
            self.spill_dev = self.torch.empty(cap, dtype=self.torch.uint8, device=self.device)

    def reserve_scan(self, nbytes, nseg):
        from . import ops
        if self.scan is None or self.scan.numel() < nbytes:
            cap = _round_up(int(nbytes * 1.25), 4096)
            self.scan = self._host(cap, self.torch.uint8)
            self.scan_dev = self.torch.empty(cap, dtype=self.torch.uint8, device=self.device) if self.cuda else None
        item = ops.jpeg_segment_dtype().itemsize
        if self.segs is None or self.segs.numel() < nseg * item:
            cap = _round_up(int(nseg * 1.25), 256) * item
            self.segs = self._host(cap, self.torch.uint8)
            self.segs_np = self.segs.numpy().view(ops.jpeg_segment_dtype())
            self.segs_dev = self.torch.empty(cap, dtype=self.torch.uint8, device=self.device) if self.cuda else None

    def wait_free(self):
        if self.event is not None:
            self.event.synchronize()
            self.event = None


class _State:
    """Everything the feeder thread touches (the DeviceLoader itself is not referenced from the thread, so dropping the
    loader lets its finalizer stop the thread)."""

    def __init__(self):
        self.stop = threading.Event()
        self.out = None
        self.thread = None
        self.pool = None
        self.cache = None                      # cache='device': the _Cache (arena + index); dropped by close()


def _put(state, item):
    while not state.stop.is_set():
        try:
            state.out.put(item, timeout=0.05)
            return True
        except queue.Full:
            pass
    return False


# ---- cache='device': decoded images resident in HBM ----------------------------------------------------------------------------
CACHE_ALIGN = 16                      # every image of the arena (and of a spill buffer) starts on a multiple of this


def source_has_miss(source, count, first_index, rank, world, cached):
    """One source file of a pass: `count` records whose global indices start at first_index.  True when a record of this
    rank (index % world == rank) is not in `cached`, a container of (source, record) keys: the file has to be opened."""
    return any((first_index + r) % world == rank and (source, r) not in cached for r in range(count))


def sources_to_open(counts, order, rank, world, cached):
    """The plan of one pass.  counts[s]: the records of source s, None while unknown; order: the pass's (shuffled) sequence
    of source indices; cached: the (source, record) keys that are resident.  Returns the sources that must be opened, in
    pass order: those holding a record of this rank that is not resident -- none for a fully cached pass -- and, from the
    first source of unknown size on, every source (the global indices behind it are unknown until it has been read)."""
    out, first = [], 0
    for k, s in enumerate(order):
        if counts[s] is None:
            return out + list(order[k:])
        if source_has_miss(s, counts[s], first, rank, world, cached):
            out.append(s)
        first += counts[s]
    return out


class _Cache:
    """The arena (one uint8 device tensor, a bump allocator, nothing is ever evicted or rewritten) and the host's index:
    (source file, record in it) -> (arena offset, height, width, text, seq_len, label, post_id, day) of a record that
    decoded and passed the max_token_id / num_classes checks."""

    def __init__(self, nbytes, device):
        import torch
        self.arena = torch.empty(int(nbytes), dtype=torch.uint8, device=device)
        self.capacity, self.used, self.full = int(nbytes), 0, False
        self.entries = {}
        self.counts = {}                       # source -> records in the file, once it has been read to its end

    def reserve(self, nbytes):
        """The arena offset of a new image, or None: once an image has found no room nothing more is inserted."""
        if self.full or self.used + nbytes > self.capacity:
            self.full = True
            return None
        off = self.used
        self.used = _round_up(off + nbytes, CACHE_ALIGN)
        return off


# ---- records ------------------------------------------------------------------------------------------------------------------
_EPOCH = object()


def _record_stream(dataset, shuffle, rng, rank, world, loop, cache=None):
    """(pass number, global index within the pass, (source, record) key, raw record or None) for the records of this rank
    in the host generator's order, _EPOCH between passes.  The source shuffle of a pass is drawn when the first record of
    that pass is asked for, never earlier.  With a cache (its `entries` and `counts`) a source whose size is known and
    whose records of this rank are all resident is not opened: its records are counted off instead; a resident record of
    an opened file carries None.  The records, their order and the draws are the same either way."""
    from .datasets.tfrecord import read_records
    index = {}
    for i, path in enumerate(dataset.data_sources):
        index.setdefault(path, i)
    pass_no = -1
    while True:
        pass_no += 1
        sources = list(dataset.data_sources)
        if shuffle:
            rng.shuffle(sources)
        idx, n = -1, 0
        for path in sources:
            s = index[path]
            count = cache.counts.get(s) if cache is not None else None
            if count is not None and not source_has_miss(s, count, idx + 1, rank, world, cache.entries):
                for r in range(count):
                    idx += 1
                    if idx % world == rank:
                        n += 1
                        yield pass_no, idx, (s, r), None
                continue
            r = -1
            for rec in read_records(path):
                idx += 1
                r += 1
                if idx % world != rank:
                    continue                   # other ranks' records: never parsed, never decoded
                n += 1
                yield pass_no, idx, (s, r), None if cache is not None and (s, r) in cache.entries else rec
            if cache is not None:
                cache.counts[s] = r + 1
        if not loop or n == 0:
            return
        yield _EPOCH


def _check_record(text, label, max_token_id, num_classes):
    if max_token_id is not None and int(np.max(text)) > max_token_id:
        raise ValueError("token id %d in the dataset exceeds the embedding table (%d rows + <ukn>): the "
                         "dataset was converted with a different vocabulary" % (int(np.max(text)), max_token_id))
    if num_classes is not None and not 0 <= label < num_classes:
        raise ValueError("label %d outside [0, %d)" % (label, num_classes))


class _Item:
    """One image of a batch.  fill: what still has to be written for it (a decoded array, JpegCoefs or JpegScan), None for
    a hit of the cache; h, w: the region the fill produces -- the crop, or under cache='device' the resident region (the
    central crop, at train time the whole image); box: the window of that region that goes to the ragged buffer (all of
    it without the cache); p: the window's TrainParams; off (cache='device'): the region's arena offset, None = spilled
    (this batch's spill buffer)."""
    __slots__ = ("off", "h", "w", "fill", "p", "box")

    def __init__(self, off, h, w, fill, p, box):
        self.off, self.h, self.w, self.fill, self.p, self.box = off, h, w, fill, p, box


def _next_item(entry, cfg, cache=None):
    """The next record of the stream, entry = (decode slot or None, pass number, global index, (source, record) key):
    awaited and checked, its image as an _Item (None with decode_images=False).  Under cache='device' a hit comes from the
    index; a miss is given its place in the arena (it is resident from here on: its pixels are written by the batch it
    belongs to, ahead of every gather that reads them on the one copy stream; a record that raises is never inserted),
    and at train time the window is drawn here -- the host generator's draws need the image's size only.  Returns the
    feeder's tuple (item, text, seq_len, label, post_id, day)."""
    slot, pass_no, idx, key = entry
    e = cache.entries.get(key) if cache is not None else None
    if e is not None:
        off, h, w, text, seq_len, label, post_id, day = e
        fill = p = None
    else:
        fill, text, seq_len, label, post_id, day = slot.result()
        _check_record(text, label, cfg.max_token_id, cfg.num_classes)
        if fill is None:
            return None, text, seq_len, label, post_id, day
        fill, p = fill if isinstance(fill, tuple) else (fill, None)
        if isinstance(fill, (JpegCoefs, JpegScan)):
            h, w, p = fill.box[2], fill.box[3], fill.params
        else:
            _check_image(fill, "input pipeline")
            h, w = fill.shape[:2]
        if p is not None and (p.crop_h, p.crop_w) != (h, w):
            raise ValueError("input pipeline: record %d is not the crop its parameters describe" % idx)
        off = None
        if cache is not None:
            off = cache.reserve(h * w * 3)
            if off is not None:
                cache.entries[key] = (off, h, w, text, seq_len, label, post_id, day)
    box = (0, 0, h, w)
    if cache is not None and cfg.train:
        box, p = _crop(h, w, (cfg.seed, pass_no, idx))
    return _Item(off, h, w, fill, p, box), text, seq_len, label, post_id, day


# ---- the batch plan: the host half of a batch -------------------------------------------------------------------------------------
_ARENA, _SPILL, _RAGGED = 0, 1, 2     # the buffers pixels are written to; the first two are the `src` values of ds_gather_desc

# used: bytes of the ragged buffer; copies: [(destination buffer, destination offset, staging offset, size)], coalesced;
# groups: [(destination buffer, first byte, one past the last byte the rows write, first ds_jpeg_desc row, rows)], arena rows
# ahead of spill rows; ncoef: int16 of coefficient storage; coef_copies: [(offset, size)] of the host-decoded coefficients;
# scans: [(ds_jpeg_desc row, JpegScan, destination buffer, destination offset, staging offset of a PIL decode, first
# coefficient)] with nscan bytes and nseg segments in the scan tables; gather: rows of the ds_ragged_gather table; arrays:
# images that arrived decoded; flagged: images the Huffman kernel flagged (flagged_fallback); stats: _CacheStats or None.
BatchPlan = collections.namedtuple("BatchPlan", "used copies groups ncoef coef_copies scans nscan nseg gather arrays flagged stats")


def pack_batch(items, out_h, out_w, st, cached=False):
    """The host half of a batch (items: _Item in output-slot order): the preprocessing descriptors of ALL images
    (st.desc_np; the ragged layout is pack_ragged's) and what puts the pixels there.  Without the cache every image is
    written straight to its ragged slot -- a decoded array is staged at the same offset of st.bytes and copied with its
    padding, so a batch of arrays is one copy of [0, used).  With it (cached) the misses are written to their place in
    the arena or the spill buffer, the arrays staged back to back, and st.gdesc_np moves every window, hit or miss, from
    there.  Coefficients go to st.coef back to back (starts rounded up to 8 int16) with one st.jdesc_np row each, the rows
    that write the arena in front of those that write the spill buffer; a JpegScan's entropy-coded bytes go to the scan
    tables (st.scan, st.sdesc_np, st.segs_np) instead.  Launches nothing; returns the BatchPlan."""
    pos = spos = stage = misses = spilled = top = 0
    pix, rows_of = [], ([], [], [])
    for i, it in enumerate(items):
        y0, x0, wh, ww = it.box
        st.desc_np[i] = _desc_record(pos, wh, ww, out_h, out_w, it.p)
        size = it.h * it.w * 3
        if not cached:
            dst, doff = _RAGGED, pos
        else:
            if it.off is None:
                dst, doff = _SPILL, spos
                spos += _round_up(size, CACHE_ALIGN)
            else:
                dst, doff = _ARENA, it.off
            st.gdesc_np[i] = (doff, pos, dst, 3 * it.w, y0, x0, wh, ww)
        pos = _round_up(pos + wh * ww * 3, 4)
        f = it.fill
        if f is None:                              # a hit: nothing is written
            continue
        misses += 1
        if dst == _SPILL:
            spilled += 1
        elif dst == _ARENA:
            top = max(top, doff + size)
        if not isinstance(f, np.ndarray):
            rows_of[dst].append((doff, size, f))
        elif cached:
            pix.append((dst, doff, stage, size, f))
            stage += _round_up(size, CACHE_ALIGN)
        else:
            pix.append((dst, doff, doff, _round_up(size, 4), f))
    # coefficient storage, ds_jpeg_desc rows and the scan list, destination buffer by destination buffer
    groups, host_coefs, scans = [], [], []
    cpos = nscan = nseg = nj = 0
    for dst in (_ARENA, _SPILL, _RAGGED):
        if not rows_of[dst]:
            continue
        base, end = 0, (spos if dst == _SPILL else pos)
        if dst == _ARENA:                          # the rows see only the bytes of the arena that this batch writes
            base, end = min(doff for doff, _, _ in rows_of[dst]), max(doff + size for doff, size, _ in rows_of[dst])
        groups.append((dst, base, end, nj, len(rows_of[dst])))
        for doff, size, f in rows_of[dst]:
            c = _round_up(cpos, 8)
            if isinstance(f, JpegScan):            # the device writes these coefficients; the PIL decode of a flagged
                soff = doff                        # image is staged at its ragged offset or, cached, behind the arrays
                if cached:
                    soff, stage = stage, stage + _round_up(size, CACHE_ALIGN)
                scans.append((nj, f, dst, doff, soff, c))
                cpos = c + f.coef_count
                nscan += int(f.cuts[-1]) - int(f.scan.scan_begin)
                nseg += f.cuts.size
            else:
                host_coefs.append((c, f.coef))
                cpos = c + f.coef.size
            st.jdesc_np[nj] = (c, doff - base, f.width, f.height, f.sampling, f.box[0], f.box[1], f.box[2], f.box[3], 0, f.quant)
            nj += 1
    st.reserve(max(pos, stage))
    st.reserve_spill(spos)
    out = st.bytes.numpy()
    copies = []
    for dst, doff, soff, size, f in pix:
        out[soff:soff + f.size].reshape(f.shape)[...] = f
        align = 4 if dst == _RAGGED else CACHE_ALIGN
        if copies and copies[-1][0] == dst and doff - copies[-1][1] == soff - copies[-1][2] == _round_up(copies[-1][3], align):
            copies[-1] = (dst, copies[-1][1], copies[-1][2], doff - copies[-1][1] + size)     # neighbours in both buffers: one copy
        else:
            copies.append((dst, doff, soff, size))
    if nj:
        st.reserve_coef(cpos)
        coef = st.coef.numpy()
        for c, a in host_coefs:
            coef[c:c + a.size] = a
    if scans:
        from . import ops
        st.reserve_scan(nscan, nseg)
        ops.fill_jpeg_scan_tables([(f.data, f.info, f.scan, f.cuts) for _, f, _, _, _, _ in scans],
                                  [c for _, _, _, _, _, c in scans], st.scan.numpy(), st.sdesc_np, st.segs_np)
    stats = _CacheStats(len(items) - misses, misses, spilled, misses - spilled, top) if cached else None
    return BatchPlan(pos, copies, groups, cpos, [(c, a.size) for c, a in host_coefs], scans, nscan, nseg,
                     len(items) if cached else 0, len(pix), 0, stats)


def flagged_fallback(plan, st, bad, whole=False):
    """Amend the plan for the images the Huffman kernel flagged (bad: their indices into plan.scans): each is decoded with
    PIL from the bytes its JpegScan holds -- the region a PIL miss has: its crop, or (whole) the uncropped image -- the
    pixels are staged in st.bytes, a copy to the image's destination is appended and its row leaves the ds_jpeg_desc
    table.  Host only: the caller issues plan.copies[len(old copies):].  Returns the new plan."""
    if not len(bad):
        return plan
    out = st.bytes.numpy()
    copies = list(plan.copies)
    keep = np.ones(sum(g[4] for g in plan.groups), bool)
    for k in bad:
        row, f, dst, doff, soff, _ = plan.scans[k]
        im = decode_pixels(f.data, f.train_key, whole)
        im = im[0] if isinstance(im, tuple) else im
        if im.shape[:2] != (f.box[2], f.box[3]):
            raise ValueError("a JPEG decodes to another size than its header states")
        out[soff:soff + im.size].reshape(im.shape)[...] = im
        copies.append((dst, doff, soff, im.size))
        keep[row] = False
    st.jdesc_np[:int(keep.sum())] = st.jdesc_np[:keep.size][keep]
    groups, nj = [], 0
    for dst, base, end, first, n in plan.groups:
        left = int(keep[first:first + n].sum())
        if left:
            groups.append((dst, base, end, nj, left))
        nj += left
    return plan._replace(copies=copies, groups=groups, flagged=len(bad))


# ---- the device half of a batch ---------------------------------------------------------------------------------------------------
def _device_entropy_launch(plan, st, stream):
    """The Huffman decode of the batch's JpegScan images on the copy stream (the current one), into their ranges of
    st.coef_dev; host-decoded images' coefficients are uploaded into theirs.  The status words come back to pinned memory
    and the FEEDER waits for them.  Returns the indices into plan.scans of the images the kernel flagged."""
    import torch
    from . import ops
    for off, size in plan.coef_copies:
        st.coef_dev[off:off + size].copy_(st.coef[off:off + size], non_blocking=True)
    ns, nscan, nseg = len(plan.scans), plan.nscan, plan.nseg
    st.scan_dev[:nscan].copy_(st.scan[:nscan], non_blocking=True)
    st.sdesc_dev.copy_(st.sdesc, non_blocking=True)
    nb = nseg * ops.jpeg_segment_dtype().itemsize
    st.segs_dev[:nb].copy_(st.segs[:nb], non_blocking=True)
    ops.jpeg_entropy_decode_device(st.scan_dev[:nscan], st.sdesc_np[:ns], st.segs_np[:nseg], st.coef_dev[:plan.ncoef],
                                   images_dev=st.sdesc_dev, segs_dev=st.segs_dev, status=st.status_dev)
    st.status[:ns].copy_(st.status_dev[:ns], non_blocking=True)
    done = torch.cuda.Event()
    done.record(stream)
    done.synchronize()
    return np.nonzero(st.status.numpy()[:ns])[0]


def _run_plan(plan, st, arena, stream, whole):
    """The device half, on the copy stream (the current one): the H2D copies of the staged pixels; the Huffman decode of
    the JpegScan images (or, without any, the upload of the coefficients); the PIL decode and upload of the images that
    kernel flagged; ds_jpeg_reconstruct once per buffer it writes -- the ragged buffer or, under cache='device', the arena
    and this staging set's spill buffer -- and then ONE ds_ragged_gather that moves every image's window, hit or miss,
    into the ragged buffer the preprocessing kernel reads.  Returns the plan as amended for the flagged images."""
    from . import ops
    bufs = (arena, st.spill_dev, st.bytes_dev)

    def upload(copies):
        for dst, doff, soff, size in copies:
            bufs[dst][doff:doff + size].copy_(st.bytes[soff:soff + size], non_blocking=True)

    upload(plan.copies)
    if plan.scans:
        issued = len(plan.copies)
        plan = flagged_fallback(plan, st, _device_entropy_launch(plan, st, stream), whole)
        upload(plan.copies[issued:])
    elif plan.groups:
        st.coef_dev[:plan.ncoef].copy_(st.coef[:plan.ncoef], non_blocking=True)
    if plan.groups:
        st.jdesc_dev.copy_(st.jdesc, non_blocking=True)
        item = ops.jpeg_desc_dtype().itemsize
        for dst, base, end, first, n in plan.groups:
            ops.jpeg_reconstruct(st.coef_dev[:plan.ncoef], st.jdesc_np[first:first + n], bufs[dst][base:end],
                                 scratch=st.scratch_dev, desc_dev=st.jdesc_dev[first * item:])
    if plan.gather:
        st.gdesc_dev.copy_(st.gdesc, non_blocking=True)
        ops.ragged_gather(arena, st.spill_dev, st.gdesc_np[:plan.gather], st.bytes_dev[:plan.used], desc_dev=st.gdesc_dev)
    return plan


def _feeder(state, dataset, cfg):
    try:
        import torch
        from . import ops
        dev, batch_size, shuffle = cfg.device, cfg.batch_size, cfg.shuffle
        cuda = dev.type == "cuda"
        if cfg.decode_images and not cuda:
            raise RuntimeError("tumblr_emotions_amd kernels need CUDA/HIP tensors; there is no CPU fallback")
        post_size = None
        stream = None
        if cuda:
            torch.cuda.set_device(dev)
            stream = torch.cuda.Stream(device=dev)
        rng = np.random.RandomState(cfg.seed)
        stagings, turn = [], 0
        pending = collections.deque()
        cache = None
        if cfg.cache_bytes:                        # cache='device': the arena lives as long as the feeder state
            cache = state.cache = _Cache(cfg.cache_bytes, dev)
        records = _record_stream(dataset, shuffle, rng, cfg.rank, cfg.world, cfg.loop, cache)
        # What a worker does with a record.  With the cache it decodes the resident region -- at train time the whole
        # image -- and the feeder draws the window (_next_item); without it the worker draws the crop from the record's key.
        decode = (decode_record_jpeg_scan if cfg.entropy else decode_record_jpeg if cfg.jpeg else
                  decode_record if cfg.decode_images else functools.partial(decode_record, decode_image=False))
        whole = cfg.train and cache is not None
        check_descs = ops.check_preprocess_train_descs if cfg.train else ops.check_preprocess_descs
        preprocess = ops.preprocess_train if cfg.train else ops.preprocess_eval
        exhausted = boundary = False
        buf = []
        while not state.stop.is_set():
            # Read ahead, but keep the RandomState's sequence equal to the host generator's: within a pass the only draws
            # are the batch permutations (made below as batches complete); the next draw after the last record of a pass is
            # the next pass's source shuffle.  So with shuffling on, the next pass starts only once every record of the
            # finished one has been consumed (a short bubble per epoch); without shuffling nothing is drawn at all.
            # With the cache a pass always waits for the one before it: what is resident is known once its records are in.
            while not exhausted and len(pending) < cfg.inflight:
                if boundary and (shuffle or cache is not None) and pending:
                    break
                boundary = False
                rec = next(records, None)
                if rec is None:
                    exhausted = True
                elif rec is _EPOCH:
                    boundary = True
                else:
                    pass_no, idx, key, payload = rec
                    slot = None                    # a hit: no file was read for it, nothing goes to the pool
                    if payload is not None:
                        slot = state.pool.submit(decode, payload, (cfg.seed, pass_no, idx) if cfg.train and cache is None else None, whole)
                    pending.append((slot, pass_no, idx, key))
            if not pending:
                break
            buf.append(_next_item(pending.popleft(), cfg, cache))
            if len(buf) < batch_size:
                continue
            order = rng.permutation(batch_size) if shuffle else np.arange(batch_size)
            if post_size is None:
                post_size = len(buf[0][1])
                stagings = [_Staging(cfg, post_size) for _ in range(max(2, cfg.prefetch + 1))]
            st = stagings[turn]
            turn = (turn + 1) % len(stagings)
            st.wait_free()
            ints = st.ints.numpy()
            nt = batch_size * post_size
            ints[:nt].reshape(batch_size, post_size)[...] = np.stack([b[1] for b in buf])[order]
            for k in range(len(_FIELDS)):
                ints[nt + k * batch_size:nt + (k + 1) * batch_size] = np.asarray([b[2 + k] for b in buf], np.int64)[order]
            plan = None
            if cfg.decode_images:                  # descriptor j = output slot j: the permutation costs nothing
                plan = pack_batch([buf[j][0] for j in order], cfg.height, cfg.width, st, cache is not None)
                check_descs(st.desc_np[:batch_size], plan.used)
            buf = []
            out = {}
            if cuda:
                with torch.cuda.stream(stream):
                    if plan is not None:
                        plan = _run_plan(plan, st, cache.arena if cache is not None else None, stream, whole)
                        st.desc_dev.copy_(st.desc, non_blocking=True)
                        out["images"] = preprocess(st.bytes_dev[:plan.used], st.desc_np[:batch_size], cfg.height, cfg.width,
                                                   desc_dev=st.desc_dev)
                    ints_dev = st.ints.to(dev, non_blocking=True)
                    st.event = torch.cuda.Event()
                    st.event.record(stream)
                event = st.event
            else:
                ints_dev, event = st.ints.clone(), None
            out["texts"] = ints_dev[:nt].view(batch_size, post_size)
            for k, (name, _) in enumerate(_FIELDS):
                out[name] = ints_dev[nt + k * batch_size:nt + (k + 1) * batch_size]
            batch = _Batch(out, event, stream, 0, 0, None)
            if plan is not None:                   # under jpeg_decode='device' an image that PIL decoded is a fallback
                batch = batch._replace(fallbacks=plan.arrays + plan.flagged if cfg.jpeg else 0,
                                       on_device=len(plan.scans) - plan.flagged, stats=plan.stats)
            if not _put(state, batch):
                return
        _put(state, None)                          # the end of the stream; an exception is handed over as itself
    except BaseException as e:
        _put(state, e)


def _shutdown(state):
    state.stop.set()
    if state.thread is not None and state.thread is not threading.current_thread():
        state.thread.join()
    if state.pool is not None:
        state.pool.close()
    state.cache = None
    try:                                       # drop queued batches (device tensors, events)
        while True:
            state.out.get_nowait()
    except queue.Empty:
        pass


def check_switches(jpeg_decode='host', jpeg_entropy='host', cache='none', cache_bytes=None):
    """The values and combinations of the device pipeline's switches, for DeviceLoader and load_batch_with_text alike."""
    if cache not in ('none', 'device'):
        raise ValueError("cache must be 'none' or 'device', not %r" % (cache,))
    if cache == 'device' and (cache_bytes is None or isinstance(cache_bytes, bool) or int(cache_bytes) < 1):
        raise ValueError("cache='device' needs an explicit positive cache_bytes: the decoded size of a dataset is not "
                         "known before it is decoded, and no share of the device memory is taken silently")
    if jpeg_decode not in ('host', 'device'):
        raise ValueError("jpeg_decode must be 'host' or 'device', not %r" % (jpeg_decode,))
    if jpeg_entropy not in ('host', 'device'):
        raise ValueError("jpeg_entropy must be 'host' or 'device', not %r" % (jpeg_entropy,))
    if jpeg_entropy == 'device' and jpeg_decode != 'device':
        raise ValueError("jpeg_entropy='device' needs jpeg_decode='device': the coefficients go to ds_jpeg_reconstruct")


class DeviceLoader:
    """Iterator over the batches of load_batch_with_text(pipeline='device').  `next(loader)` makes the current stream
    wait for the batch's upload + preprocessing (an event; the host is not blocked by the device) and returns the dict.
    close() -- also run by the context manager, by garbage collection of the loader and at interpreter exit -- stops the
    feeder and joins every worker; a closed or exhausted loader raises StopIteration.  is_training=True: the train-time
    augmentation (ds_preprocess_train) instead of the eval chain; ignored with decode_images=False.  jpeg_decode='device':
    compiled Huffman decode in the workers and ds_jpeg_reconstruct on the copy stream instead of PIL (ignored with
    decode_images=False); jpeg_fallbacks counts the images of the batches handed out so far that took the PIL path.
    jpeg_entropy='device' (with jpeg_decode='device' only, a ValueError otherwise): the Huffman decode of restart-segmented
    streams in ds_jpeg_entropy_decode_device as well; jpeg_device_entropy counts the images whose coefficients the device
    produced, and an image the kernel flags is a fallback.  cache='device' with cache_bytes (a positive number of bytes, no
    default; a ValueError without it, and on a device that is not CUDA/HIP unless decode_images=False, where the switch does
    nothing): decoded images stay in an arena of that size and later passes are assembled from it by ds_ragged_gather --
    the same batches; cache_stats() reports, close() frees the arena."""

    def __init__(self, dataset, batch_size=32, shuffle=True, height=299, width=299, is_training=False, device="cuda",
                 rank=0, world=1, seed=0, loop=True, max_token_id=None, num_classes=None, workers=8, prefetch=2,
                 decode_images=True, jpeg_decode='host', jpeg_entropy='host', cache='none', cache_bytes=None):
        check_switches(jpeg_decode, jpeg_entropy, cache, cache_bytes)
        self.jpeg_decode, self.jpeg_entropy = jpeg_decode, jpeg_entropy
        self.jpeg_fallbacks = 0
        self.jpeg_device_entropy = 0
        self.cache = cache
        if batch_size < 1 or height < 1 or width < 1 or world < 1 or not 0 <= rank < world:
            raise ValueError("DeviceLoader: bad batch_size / height / width / rank / world")
        self.workers = clamp_workers(workers)
        self.prefetch = max(1, int(prefetch))
        self.decode_images = bool(decode_images)
        self._done = False
        import torch
        device = torch.device(device)
        if device.type == "cuda" and device.index is None and torch.cuda.is_available():
            device = torch.device("cuda", torch.cuda.current_device())      # the caller's current device, not the feeder thread's
        if cache == 'device' and self.decode_images and device.type != "cuda":
            raise ValueError("cache='device' needs a CUDA/HIP device: the arena is device memory")
        jpeg = self.decode_images and jpeg_decode == 'device'
        cfg = _Config(int(batch_size), int(height), int(width), device, self.decode_images,
                      train=self.decode_images and bool(is_training), jpeg=jpeg, entropy=jpeg and jpeg_entropy == 'device',
                      cache_bytes=int(cache_bytes) if cache == 'device' and self.decode_images else None,
                      shuffle=bool(shuffle), rank=rank, world=world, seed=seed, loop=bool(loop), max_token_id=max_token_id,
                      num_classes=num_classes, prefetch=self.prefetch,
                      inflight=max(4 * self.workers, min(int(batch_size), 256)))
        self._cache_stats = {'hits': 0, 'misses': 0, 'spilled': 0, 'bytes_used': 0, 'records': 0,
                             'bytes_capacity': cfg.cache_bytes or 0}
        st = self._state = _State()
        st.out = queue.Queue(maxsize=self.prefetch)
        st.pool = OrderedPool(self.workers)
        st.thread = threading.Thread(target=_feeder, name="ds-input-feeder", daemon=True, args=(st, dataset, cfg))
        self._finalizer = weakref.finalize(self, _shutdown, st)
        st.thread.start()

    def __iter__(self):
        return self

    def __next__(self):
        if self._done:
            raise StopIteration
        item = self._state.out.get()
        if isinstance(item, _Batch):
            self.jpeg_fallbacks += item.fallbacks
            self.jpeg_device_entropy += item.on_device
            if item.stats is not None:
                c = self._cache_stats
                for k in ('hits', 'misses', 'spilled', 'records'):
                    c[k] += getattr(item.stats, k)
                c['bytes_used'] = max(c['bytes_used'], item.stats.bytes_used)
            if item.event is not None:
                import torch
                cur = torch.cuda.current_stream(item.stream.device)
                cur.wait_event(item.event)
                for t in item.out.values():     # allocated on the copy stream, consumed (and later freed) on this one
                    t.record_stream(cur)
            return item.out
        self.close()
        if item is not None:                    # the feeder's exception; None is the end of the stream
            raise item
        raise StopIteration

    def close(self):
        self._done = True
        self._finalizer()

    def cache_stats(self):
        """The decoded-image cache over the batches handed out so far: images served from the arena (hits), images decoded
        (misses), of those the ones that found no room and went through a spill buffer (spilled), the arena bytes in use
        and its size, and the records resident.  All zero with cache='none' (or decode_images=False)."""
        return dict(self._cache_stats)

    def threads(self):
        """The loader's live threads (feeder + decode workers); empty after close()."""
        st = self._state
        ts = ([st.thread] if st.thread is not None else []) + list(st.pool._threads)
        return [t for t in ts if t.is_alive()]

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False
