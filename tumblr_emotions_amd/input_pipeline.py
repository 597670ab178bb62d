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
"""
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
        if im.ndim != 3 or im.shape[2] != 3 or im.dtype != np.uint8 or im.shape[0] < 1 or im.shape[1] < 1:
            raise ValueError("pack_ragged: images must be non-empty uint8 [h, w, 3] arrays")
        offsets.append(pos)
        pos = -(-(pos + im.size) // align) * align
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


def decode_record(rec, decode_image=True, train_key=None, whole=False):
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
    if whole:
        return np.ascontiguousarray(img)
    if train_key is None:
        y0, x0, ch, cw = crop_box(img.shape[0], img.shape[1])
        return np.ascontiguousarray(img[y0:y0 + ch, x0:x0 + cw])
    from .preprocessing.inception_preprocessing import record_rng, sample_train_params
    p = sample_train_params(img.shape[0], img.shape[1], record_rng(*train_key))
    return np.ascontiguousarray(img[p.y0:p.y0 + p.crop_h, p.x0:p.x0 + p.crop_w]), p


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
    if whole:
        box, p = (0, 0, h, w), None
    elif train_key is None:
        box, p = crop_box(h, w), None
    else:
        from .preprocessing.inception_preprocessing import record_rng, sample_train_params
        p = sample_train_params(h, w, record_rng(*train_key))
        box = (p.y0, p.x0, p.crop_h, p.crop_w)
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
        return decode_record(rec, True, train_key, whole)
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


def pack_ragged_jpeg(items, out_h, out_w, st, train=False):
    """pack_ragged for a batch whose items are JpegCoefs or decoded crops (train: (crop, TrainParams)): the preprocessing
    descriptors of ALL images and the pixels of the decoded ones go where pack_ragged puts them (st.desc_np, st.bytes);
    coefficients go to st.coef back to back (starts rounded up to 8 int16) with one st.jdesc_np record each.  Returns
    (bytes used, int16 used, JpegCoefs count, [(offset, size) of every decoded crop])."""
    shapes, pos, cpos, spos, nseg = [], 0, 0, 0, 0
    for it in items:
        if isinstance(it, JpegCoefs):
            ch, cw = it.box[2], it.box[3]
            cpos = -(-cpos // 8) * 8 + it.coef.size
        elif isinstance(it, JpegScan):
            ch, cw = it.box[2], it.box[3]
            cpos = -(-cpos // 8) * 8 + it.coef_count
            spos += int(it.cuts[-1]) - int(it.scan.scan_begin)
            nseg += it.cuts.size
        else:
            im = it[0] if train else it
            if im.ndim != 3 or im.shape[2] != 3 or im.dtype != np.uint8 or im.shape[0] < 1 or im.shape[1] < 1:
                raise ValueError("pack_ragged_jpeg: images must be non-empty uint8 [h, w, 3] arrays")
            ch, cw = im.shape[:2]
        shapes.append((pos, ch, cw))
        pos = -(-(pos + ch * cw * 3) // 4) * 4
    st.reserve(pos)
    st.reserve_coef(cpos)
    if nseg:
        st.reserve_scan(spos, nseg)
    out, coef = st.bytes.numpy(), st.coef.numpy()
    cpos, nj, copies = 0, 0, []
    st.scans, st.coef_copies = [], []
    for i, (it, (off, ch, cw)) in enumerate(zip(items, shapes)):
        if isinstance(it, (JpegCoefs, JpegScan)):
            p = it.params
            cpos = -(-cpos // 8) * 8
            if isinstance(it, JpegCoefs):
                size = it.coef.size
                coef[cpos:cpos + size] = it.coef
                st.coef_copies.append((cpos, size))
            else:                                  # the device writes these coefficients: (descriptor row, item, byte offset)
                size = it.coef_count
                st.scans.append((nj, it, off, cpos))
            st.jdesc_np[nj] = (cpos, off, it.width, it.height, it.sampling, it.box[0], it.box[1], ch, cw, 0, it.quant)
            cpos += size
            nj += 1
        else:
            im, p = it if train else (it, None)
            out[off:off + im.size].reshape(im.shape)[...] = im
            copies.append((off, im.size))
        if train and (p.crop_h, p.crop_w) != (ch, cw):
            raise ValueError("pack_ragged_jpeg: image %d is not the crop its parameters describe" % i)
        st.desc_np[i] = _desc_record(off, ch, cw, out_h, out_w, p if train else None)
    if st.scans:
        from . import ops
        ops.fill_jpeg_scan_tables([(it.data, it.info, it.scan, it.cuts) for _, it, _, _ in st.scans],
                                  [c for _, _, _, c in st.scans], st.scan.numpy(), st.sdesc_np, st.segs_np)
        st.scan_used, st.segs_used = spos, nseg
    return pos, cpos, nj, copies


# ---- staging ----------------------------------------------------------------------------------------------------------------
class _Staging:
    """One pinned staging set: ragged image bytes + descriptor table + the int64 fields, with the device byte buffer and
    descriptor table they are uploaded into and the event of the last upload."""

    def __init__(self, batch_size, post_size, device, cuda, train=False, jpeg=False, entropy=False, cache=False):
        import torch
        from . import ops
        preprocess_desc_dtype = ops.preprocess_train_desc_dtype if train else ops.preprocess_desc_dtype
        self.torch, self.device, self.cuda = torch, device, cuda
        self.event = None
        self.ints = self._host(batch_size * (post_size + len(_FIELDS)), torch.int64)
        self.desc = self._host(batch_size * preprocess_desc_dtype().itemsize, torch.uint8)
        self.desc_np = self.desc.numpy().view(preprocess_desc_dtype())
        self.desc_dev = torch.empty(self.desc.numel(), dtype=torch.uint8, device=device) if cuda else None
        self.bytes = self.bytes_dev = None
        self.reserve(1 << 20)
        self.coef = self.coef_dev = self.scratch_dev = None
        if jpeg:                  # jpeg_decode='device': coefficients, their descriptors, the planes of ds_jpeg_reconstruct
            self.jdesc = self._host(batch_size * ops.jpeg_desc_dtype().itemsize, torch.uint8)
            self.jdesc_np = self.jdesc.numpy().view(ops.jpeg_desc_dtype())
            self.jdesc_dev = torch.empty(self.jdesc.numel(), dtype=torch.uint8, device=device) if cuda else None
            self.reserve_coef(1 << 20)
        self.scans, self.coef_copies = [], []     # pack_ragged_jpeg: the JpegScan images, the ranges of host-decoded coefficients
        self.scan = self.scan_dev = self.segs = self.segs_np = self.segs_dev = None
        if jpeg and entropy:      # jpeg_entropy='device': entropy-coded bytes, the two tables, the status words
            self.sdesc = self._host(batch_size * ops.jpeg_scan_desc_dtype().itemsize, torch.uint8)
            self.sdesc_np = self.sdesc.numpy().view(ops.jpeg_scan_desc_dtype())
            self.status = self._host(batch_size, torch.int32)
            if cuda:
                self.sdesc_dev = torch.empty(self.sdesc.numel(), dtype=torch.uint8, device=device)
                self.status_dev = torch.empty(batch_size, dtype=torch.int32, device=device)
            self.reserve_scan(1 << 20, 1 << 12)
        self.spill_dev = None
        if cache:                 # cache='device': the ds_ragged_gather table; the spill buffer appears with the first spilled image
            self.gdesc = self._host(batch_size * ops.gather_desc_dtype().itemsize, torch.uint8)
            self.gdesc_np = self.gdesc.numpy().view(ops.gather_desc_dtype())
            self.gdesc_dev = torch.empty(self.gdesc.numel(), dtype=torch.uint8, device=device)

    def _host(self, n, dtype):
        return self.torch.empty(n, dtype=dtype, pin_memory=self.cuda)

    def reserve(self, nbytes):
        if self.bytes is None or self.bytes.numel() < nbytes:
            cap = -(-int(nbytes * 1.25) // 4096) * 4096
            self.bytes = self._host(cap, self.torch.uint8)
            self.bytes_dev = self.torch.empty(cap, dtype=self.torch.uint8, device=self.device) if self.cuda else None

    def reserve_coef(self, n):
        if self.coef is None or self.coef.numel() < n:
            cap = -(-int(n * 1.25) // 4096) * 4096
            self.coef = self._host(cap, self.torch.int16)
            if self.cuda:
                self.coef_dev = self.torch.empty(cap, dtype=self.torch.int16, device=self.device)
                self.scratch_dev = self.torch.empty(cap, dtype=self.torch.uint8, device=self.device)

    def reserve_spill(self, nbytes):
        if nbytes and (self.spill_dev is None or self.spill_dev.numel() < nbytes):
            cap = -(-int(nbytes * 1.25) // 4096) * 4096
            self.spill_dev = self.torch.empty(cap, dtype=self.torch.uint8, device=self.device)

    def reserve_scan(self, nbytes, nseg):
        from . import ops
        if self.scan is None or self.scan.numel() < nbytes:
            cap = -(-int(nbytes * 1.25) // 4096) * 4096
            self.scan = self._host(cap, self.torch.uint8)
            self.scan_dev = self.torch.empty(cap, dtype=self.torch.uint8, device=self.device) if self.cuda else None
        item = ops.jpeg_segment_dtype().itemsize
        if self.segs is None or self.segs.numel() < nseg * item:
            cap = -(-int(nseg * 1.25) // 256) * 256 * item
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


_EPOCH = object()


def _record_stream(dataset, shuffle, rng, rank, world, loop):
    """(pass number, global index within the pass, raw record) for the records of this rank in the host generator's order,
    _EPOCH between passes.  The source shuffle of a pass is drawn when the first record of that pass is asked for, never
    earlier."""
    from .datasets.tfrecord import read_records
    pass_no = -1
    while True:
        pass_no += 1
        sources = list(dataset.data_sources)
        if shuffle:
            rng.shuffle(sources)
        idx, n = -1, 0
        for path in sources:
            for rec in read_records(path):
                idx += 1
                if idx % world != rank:
                    continue                   # other ranks' records: never parsed, never decoded
                n += 1
                yield pass_no, idx, rec
        if not loop or n == 0:
            return
        yield _EPOCH


# ---- cache='device': decoded images resident in HBM ----------------------------------------------------------------------------
CACHE_ALIGN = 16                      # every image of the arena (and of a spill buffer) starts on a multiple of this


def _round_up(n, m):
    return -(-n // m) * m


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


class _CacheItem:
    """One image of a batch under cache='device'.  off: its arena offset, None = spilled (this batch's spill buffer);
    h, w: the resident region (the central crop, at train time the whole image); fill: what still has to be written there
    (a decoded array, JpegCoefs or JpegScan), None for a hit; box: the window ds_ragged_gather copies; p: its TrainParams."""
    __slots__ = ("off", "h", "w", "fill", "p", "box", "hit")

    def __init__(self, off, h, w, fill, p, box):
        self.off, self.h, self.w, self.fill, self.p, self.box, self.hit = off, h, w, fill, p, box, fill is None


def _cached_record_stream(dataset, shuffle, rng, rank, world, loop, cache):
    """_record_stream under cache='device': (pass number, global index, (source, record) key, raw record or None), the
    same records in the same order with the same draws.  A source whose size is known and whose records of this rank are
    all resident is not opened: its records are counted off instead; a resident record of an opened file carries None."""
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
            count = cache.counts.get(s)
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
                    continue
                n += 1
                yield pass_no, idx, (s, r), None if (s, r) in cache.entries else rec
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


def _cache_pop(cache, entry, train, seed, max_token_id, num_classes):
    """The next record of the stream under cache='device': a hit comes from the index; a miss is awaited, checked and given
    its place in the arena (it is resident from here on: its pixels are written by the batch it belongs to, ahead of every
    gather that reads them on the one copy stream).  A record that raises is never inserted.  Returns the feeder's tuple,
    its first item a _CacheItem."""
    slot, pass_no, idx, key = entry
    e = cache.entries.get(key)
    fill = None
    if e is None:
        fill, text, seq_len, label, post_id, day = slot.result()
        _check_record(text, label, max_token_id, num_classes)
        h, w = (fill.box[2], fill.box[3]) if isinstance(fill, (JpegCoefs, JpegScan)) else fill.shape[:2]
        off = cache.reserve(h * w * 3)
        if off is not None:
            cache.entries[key] = (off, h, w, text, seq_len, label, post_id, day)
    else:
        off, h, w, text, seq_len, label, post_id, day = e
    p, box = None, (0, 0, h, w)
    if train:                                      # the host generator's draws: they need the image's size only
        from .preprocessing.inception_preprocessing import record_rng, sample_train_params
        p = sample_train_params(h, w, record_rng(seed, pass_no, idx))
        box = (p.y0, p.x0, p.crop_h, p.crop_w)
    return _CacheItem(off, h, w, fill, p, box), text, seq_len, label, post_id, day


def _pack_cached(items, out_h, out_w, st):
    """The host half of a batch under cache='device' (items in output-slot order): the ds_ragged_gather table and the
    preprocessing descriptors of ALL images (st.gdesc_np, st.desc_np; the ragged layout is pack_ragged's), and for the
    misses what puts their pixels where the gather reads them -- decoded arrays into pinned staging (st.bytes), coefficients
    and ds_jpeg_desc rows as pack_ragged_jpeg lays them out, the rows that write the arena in front of those that write the
    spill buffer.  Returns (ragged bytes, int16 used, arena rows, rows, [(src, destination offset, staging offset, size)
    of every staged array], (first, one past the last) arena byte the rows write, staging offset free for fallbacks)."""
    pos = spos = stage = room = 0
    pix, rows_of = [], ([], [])
    for i, it in enumerate(items):
        size = it.h * it.w * 3
        if it.off is None:
            src, soff = 1, spos
            spos += _round_up(size, CACHE_ALIGN)
        else:
            src, soff = 0, it.off
        y0, x0, wh, ww = it.box
        st.gdesc_np[i] = (soff, pos, src, 3 * it.w, y0, x0, wh, ww)
        st.desc_np[i] = _desc_record(pos, wh, ww, out_h, out_w, it.p)
        pos = _round_up(pos + wh * ww * 3, 4)
        f, it.fill = it.fill, None
        if isinstance(f, (JpegCoefs, JpegScan)):
            rows_of[src].append((soff, f))
            if isinstance(f, JpegScan):
                room += _round_up(size, CACHE_ALIGN)           # for the PIL decode of an image the kernel flags
        elif f is not None:
            if f.ndim != 3 or f.shape[2] != 3 or f.dtype != np.uint8 or f.shape[0] < 1 or f.shape[1] < 1:
                raise ValueError("input cache: images must be non-empty uint8 [h, w, 3] arrays")
            pix.append((src, soff, stage, f))
            stage += _round_up(size, CACHE_ALIGN)
    st.reserve(max(pos, stage + room))
    st.reserve_spill(spos)
    out = st.bytes.numpy()
    copies = []
    for src, doff, sp, f in pix:
        out[sp:sp + f.size].reshape(f.shape)[...] = f
        if copies and copies[-1][0] == src and doff - copies[-1][1] == sp - copies[-1][2] == _round_up(copies[-1][3], CACHE_ALIGN):
            copies[-1] = (src, copies[-1][1], copies[-1][2], doff - copies[-1][1] + f.size)     # neighbours in both buffers: one copy
        else:
            copies.append((src, doff, sp, f.size))
    rows, na = rows_of[0] + rows_of[1], len(rows_of[0])
    abase = min((off for off, _ in rows_of[0]), default=0)
    aend = max((off + f.box[2] * f.box[3] * 3 for off, f in rows_of[0]), default=0)
    cpos = nscan = nseg = 0
    for _, f in rows:
        if isinstance(f, JpegCoefs):
            cpos = _round_up(cpos, 8) + f.coef.size
        else:
            cpos = _round_up(cpos, 8) + f.coef_count
            nscan += int(f.cuts[-1]) - int(f.scan.scan_begin)
            nseg += f.cuts.size
    st.scans, st.coef_copies = [], []
    if rows:
        st.reserve_coef(cpos)
        if nseg:
            st.reserve_scan(nscan, nseg)
        coef, cpos = st.coef.numpy(), 0
        for nj, (doff, f) in enumerate(rows):
            cpos = _round_up(cpos, 8)
            if isinstance(f, JpegCoefs):
                size = f.coef.size
                coef[cpos:cpos + size] = f.coef
                st.coef_copies.append((cpos, size))
            else:                                  # (descriptor row, item, (src, destination offset), first coefficient)
                size = f.coef_count
                st.scans.append((nj, f, (0 if nj < na else 1, doff), cpos))
            st.jdesc_np[nj] = (cpos, doff - abase if nj < na else doff, f.width, f.height, f.sampling, f.box[0], f.box[1],
                               f.box[2], f.box[3], 0, f.quant)
            cpos += size
        if st.scans:
            from . import ops
            ops.fill_jpeg_scan_tables([(f.data, f.info, f.scan, f.cuts) for _, f, _, _ in st.scans],
                                      [c for _, _, _, c in st.scans], st.scan.numpy(), st.sdesc_np, st.segs_np)
            st.scan_used, st.segs_used = nscan, nseg
    return pos, cpos, na, len(rows), copies, (abase, aend), stage


def _fill_cached(st, cache, plan, stream, train, batch_size):
    """The device half, on the copy stream (the current one): the misses' pixels into the arena -- or, for a spilled image,
    into this staging set's spill buffer -- by H2D copies and ds_jpeg_reconstruct, then ONE ds_ragged_gather that moves
    every image's window, hit or miss, into the ragged buffer the preprocessing kernel reads.  Returns (images of the
    batch PIL decoded because the Huffman kernel flagged them, images whose coefficients the device produced)."""
    from . import ops
    used, ncoef, na, nj, copies, (abase, aend), free = plan
    arena = cache.arena
    for src, doff, sp, size in copies:
        (st.spill_dev if src else arena)[doff:doff + size].copy_(st.bytes[sp:sp + size], non_blocking=True)
    flagged = on_device = 0
    if st.scans:
        bad = _device_entropy_launch(st, stream, ncoef)
        keep = np.ones(nj, bool)
        out = st.bytes.numpy()
        for k in bad:
            row, it, (src, doff), _ = st.scans[k]
            im = decode_pixels(it.data, None, whole=train)             # the resident region, as a miss of the PIL path has it
            if im.shape[:2] != (it.box[2], it.box[3]):
                raise ValueError("a JPEG decodes to another size than its header states")
            out[free:free + im.size].reshape(im.shape)[...] = im
            (st.spill_dev if src else arena)[doff:doff + im.size].copy_(st.bytes[free:free + im.size], non_blocking=True)
            free += _round_up(im.size, CACHE_ALIGN)
            keep[row] = False
        flagged, on_device = int(bad.size), len(st.scans) - int(bad.size)
        if flagged:
            st.jdesc_np[:int(keep.sum())] = st.jdesc_np[:nj][keep]
            na, nj = int(keep[:na].sum()), int(keep.sum())
    elif nj:
        st.coef_dev[:ncoef].copy_(st.coef[:ncoef], non_blocking=True)
    if nj:
        st.jdesc_dev.copy_(st.jdesc, non_blocking=True)
        item = ops.jpeg_desc_dtype().itemsize
        if na:
            ops.jpeg_reconstruct(st.coef_dev[:ncoef], st.jdesc_np[:na], arena[abase:aend], scratch=st.scratch_dev,
                                 desc_dev=st.jdesc_dev)
        if nj > na:
            ops.jpeg_reconstruct(st.coef_dev[:ncoef], st.jdesc_np[na:nj], st.spill_dev, scratch=st.scratch_dev,
                                 desc_dev=st.jdesc_dev[na * item:])
    st.gdesc_dev.copy_(st.gdesc, non_blocking=True)
    ops.ragged_gather(arena, st.spill_dev, st.gdesc_np[:batch_size], st.bytes_dev[:used], desc_dev=st.gdesc_dev)
    return flagged, on_device


def _feeder(state, dataset, batch_size, shuffle, height, width, device, rank, world, seed, loop, max_token_id,
            num_classes, decode_images, prefetch, inflight, train=False, jpeg=False, entropy=False, cache_bytes=None):
    import collections
    try:
        import torch
        from . import ops
        dev = torch.device(device)
        cuda = dev.type == "cuda"
        if decode_images and not cuda:
            raise RuntimeError("tumblr_emotions_amd kernels need CUDA/HIP tensors; there is no CPU fallback")
        post_size = None
        stream = None
        if cuda:
            torch.cuda.set_device(dev)
            stream = torch.cuda.Stream(device=dev)
        rng = np.random.RandomState(seed)
        stagings, turn = [], 0
        pending = collections.deque()
        cache = None
        if cache_bytes and decode_images:          # cache='device': the arena lives as long as the feeder state
            cache = state.cache = _Cache(cache_bytes, dev)
            records = _cached_record_stream(dataset, shuffle, rng, rank, world, loop, cache)
        else:
            records = _record_stream(dataset, shuffle, rng, rank, world, loop)
        exhausted = boundary = False
        buf = []
        while not state.stop.is_set():
            # Read ahead, but keep the RandomState's sequence equal to the host generator's: within a pass the only draws
            # are the batch permutations (made below as batches complete); the next draw after the last record of a pass is
            # the next pass's source shuffle.  So with shuffling on, the next pass starts only once every record of the
            # finished one has been consumed (a short bubble per epoch); without shuffling nothing is drawn at all.
            # With the cache a pass always waits for the one before it: what is resident is known once its records are in.
            while not exhausted and len(pending) < inflight:
                if boundary and (shuffle or cache is not None) and pending:
                    break
                boundary = False
                rec = next(records, None)
                if rec is None:
                    exhausted = True
                elif rec is _EPOCH:
                    boundary = True
                elif cache is not None:
                    pass_no, idx, ckey, payload = rec
                    slot = None                    # a hit: no file was read for it, nothing goes to the pool
                    if payload is not None and jpeg:
                        slot = state.pool.submit(decode_record_jpeg_scan if entropy else decode_record_jpeg, payload, None, train)
                    elif payload is not None:
                        slot = state.pool.submit(decode_record, payload, True, None, train)
                    pending.append((slot, pass_no, idx, ckey))
                else:
                    pass_no, idx, payload = rec
                    key = (seed, pass_no, idx) if train and decode_images else None
                    if jpeg and decode_images:
                        pending.append(state.pool.submit(decode_record_jpeg_scan if entropy else decode_record_jpeg, payload, key))
                    else:
                        pending.append(state.pool.submit(decode_record, payload, decode_images, key))
            if not pending:
                break
            if cache is not None:
                img, text, seq_len, label, post_id, day = _cache_pop(cache, pending.popleft(), train, seed, max_token_id, num_classes)
            else:
                img, text, seq_len, label, post_id, day = pending.popleft().result()
                _check_record(text, label, max_token_id, num_classes)
            buf.append((img, text, seq_len, label, post_id, day))
            if len(buf) < batch_size:
                continue
            order = rng.permutation(batch_size) if shuffle else np.arange(batch_size)
            if post_size is None:
                post_size = len(buf[0][1])
                stagings = [_Staging(batch_size, post_size, dev, cuda, train and decode_images, jpeg and decode_images, entropy,
                                     cache is not None)
                            for _ in range(max(2, prefetch + 1))]
            st = stagings[turn]
            turn = (turn + 1) % len(stagings)
            st.wait_free()
            ints = st.ints.numpy()
            nt = batch_size * post_size
            ints[:nt].reshape(batch_size, post_size)[...] = np.stack([b[1] for b in buf])[order]
            for k in range(len(_FIELDS)):
                ints[nt + k * batch_size:nt + (k + 1) * batch_size] = np.asarray([b[2 + k] for b in buf], np.int64)[order]
            used = ncoef = njpeg = 0
            copies = []
            plan = cstats = None
            if cache is not None:
                items = [buf[j][0] for j in order]
                fresh = [it for it in items if not it.hit]
                kept = [it for it in fresh if it.off is not None]
                cstats = (len(items) - len(fresh), len(fresh), len(fresh) - len(kept), len(kept),
                          max((it.off + it.h * it.w * 3 for it in kept), default=0), sum(isinstance(it.fill, np.ndarray) for it in fresh))
                plan = _pack_cached(items, height, width, st)
                used = plan[0]
                (ops.check_preprocess_train_descs if train else ops.check_preprocess_descs)(st.desc_np[:batch_size], used)
            elif decode_images and jpeg:
                used, ncoef, njpeg, copies = pack_ragged_jpeg([buf[j][0] for j in order], height, width, st, train)
                (ops.check_preprocess_train_descs if train else ops.check_preprocess_descs)(st.desc_np[:batch_size], used)
                if njpeg:
                    ops.check_jpeg_descs(st.jdesc_np[:njpeg], ncoef, used)
            elif decode_images:
                images = [buf[j][0] for j in order]          # descriptor j = output slot j: the permutation costs nothing
                params = None
                if train:
                    images, params = [im for im, _ in images], [p for _, p in images]
                st.reserve(sum(-(-im.size // 4) * 4 for im in images))
                _, _, used = pack_ragged(images, height, width, out=st.bytes.numpy(), desc=st.desc_np, params=params)
                (ops.check_preprocess_train_descs if train else ops.check_preprocess_descs)(st.desc_np[:batch_size], used)
            buf = []
            out = {}
            flagged = on_device = 0
            if cuda:
                with torch.cuda.stream(stream):
                    if cache is not None:
                        flagged, on_device = _fill_cached(st, cache, plan, stream, train, batch_size)
                    elif decode_images and jpeg:
                        for off, size in copies:                 # the images PIL decoded: their slots only
                            st.bytes_dev[off:off + size].copy_(st.bytes[off:off + size], non_blocking=True)
                        if st.scans:
                            njpeg, flagged = _device_entropy(st, stream, ncoef, njpeg, train)
                            on_device = len(st.scans) - flagged
                        elif njpeg:
                            st.coef_dev[:ncoef].copy_(st.coef[:ncoef], non_blocking=True)
                        if njpeg:
                            st.jdesc_dev.copy_(st.jdesc, non_blocking=True)
                            ops.jpeg_reconstruct(st.coef_dev[:ncoef], st.jdesc_np[:njpeg], st.bytes_dev[:used],
                                                 scratch=st.scratch_dev, desc_dev=st.jdesc_dev)
                    elif decode_images:
                        st.bytes_dev[:used].copy_(st.bytes[:used], non_blocking=True)
                    if decode_images:
                        st.desc_dev.copy_(st.desc, non_blocking=True)
                        run = ops.preprocess_train if train else ops.preprocess_eval
                        out["images"] = run(st.bytes_dev[:used], st.desc_np[:batch_size], height, width, desc_dev=st.desc_dev)
                    ints_dev = st.ints.to(dev, non_blocking=True)
                    st.event = torch.cuda.Event()
                    st.event.record(stream)
                event = st.event
            else:
                ints_dev, event = st.ints.clone(), None
            out["texts"] = ints_dev[:nt].view(batch_size, post_size)
            for k, (name, _) in enumerate(_FIELDS):
                out[name] = ints_dev[nt + k * batch_size:nt + (k + 1) * batch_size]
            fallbacks = (cstats[5] if cache is not None else len(copies)) + flagged if jpeg else 0
            if not _put(state, ("batch", out, event, stream, fallbacks, on_device, cstats)):
                return
        _put(state, ("end",))
    except BaseException as e:
        _put(state, ("error", e))


def _device_entropy_launch(st, stream, ncoef):
    """The Huffman decode of the batch's JpegScan images on the copy stream (the current one), into their ranges of
    st.coef_dev; host-decoded images' coefficients are uploaded into theirs.  The status words come back to pinned memory
    and the FEEDER waits for them.  Returns the indices into st.scans of the images the kernel flagged."""
    import torch
    from . import ops
    for off, size in st.coef_copies:
        st.coef_dev[off:off + size].copy_(st.coef[off:off + size], non_blocking=True)
    ns, nscan, nseg = len(st.scans), st.scan_used, st.segs_used
    st.scan_dev[:nscan].copy_(st.scan[:nscan], non_blocking=True)
    st.sdesc_dev.copy_(st.sdesc, non_blocking=True)
    nb = nseg * ops.jpeg_segment_dtype().itemsize
    st.segs_dev[:nb].copy_(st.segs[:nb], non_blocking=True)
    ops.jpeg_entropy_decode_device(st.scan_dev[:nscan], st.sdesc_np[:ns], st.segs_np[:nseg], st.coef_dev[:ncoef],
                                   images_dev=st.sdesc_dev, segs_dev=st.segs_dev, status=st.status_dev)
    st.status[:ns].copy_(st.status_dev[:ns], non_blocking=True)
    done = torch.cuda.Event()
    done.record(stream)
    done.synchronize()
    return np.nonzero(st.status.numpy()[:ns])[0]


def _device_entropy(st, stream, ncoef, njpeg, train):
    """_device_entropy_launch for a batch without the cache: a flagged image is decoded with PIL from the bytes it holds,
    its crop uploaded into its slot of the ragged buffer and its row dropped from the reconstruct table.  Returns (rows
    left in st.jdesc_np, flagged)."""
    bad = _device_entropy_launch(st, stream, ncoef)
    if not bad.size:
        return njpeg, 0
    keep = np.ones(njpeg, bool)
    out = st.bytes.numpy()
    for k in bad:
        row, it, off, _ = st.scans[k]
        im = decode_pixels(it.data, it.train_key)
        im = im[0] if train else im
        if im.shape[:2] != (it.box[2], it.box[3]):
            raise ValueError("a JPEG decodes to another size than its header states")
        out[off:off + im.size].reshape(im.shape)[...] = im
        st.bytes_dev[off:off + im.size].copy_(st.bytes[off:off + im.size], non_blocking=True)
        keep[row] = False
    left = int(keep.sum())
    st.jdesc_np[:left] = st.jdesc_np[:njpeg][keep]
    return left, int(bad.size)




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
        self.jpeg_decode, self.jpeg_entropy = jpeg_decode, jpeg_entropy
        self.jpeg_fallbacks = 0
        self.jpeg_device_entropy = 0
        self.cache = cache
        self._cache_stats = {'hits': 0, 'misses': 0, 'spilled': 0, 'bytes_used': 0, 'records': 0,
                             'bytes_capacity': int(cache_bytes) if cache == 'device' and decode_images else 0}
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
        st = self._state = _State()
        st.out = queue.Queue(maxsize=self.prefetch)
        st.pool = OrderedPool(self.workers)
        inflight = max(4 * self.workers, min(int(batch_size), 256))
        st.thread = threading.Thread(target=_feeder, name="ds-input-feeder", daemon=True,
                                     args=(st, dataset, int(batch_size), bool(shuffle), int(height), int(width), device, rank,
                                           world, seed, bool(loop), max_token_id, num_classes, self.decode_images,
                                           self.prefetch, inflight, bool(is_training), jpeg_decode == 'device',
                                           jpeg_entropy == 'device',
                                           int(cache_bytes) if cache == 'device' and self.decode_images else None))
        self._finalizer = weakref.finalize(self, _shutdown, st)
        st.thread.start()

    def __iter__(self):
        return self

    def __next__(self):
        if self._done:
            raise StopIteration
        item = self._state.out.get()
        if item[0] == "batch":
            _, out, event, stream, fallbacks, on_device, cstats = item
            self.jpeg_fallbacks += fallbacks
            self.jpeg_device_entropy += on_device
            if cstats is not None:
                c = self._cache_stats
                c['hits'] += cstats[0]
                c['misses'] += cstats[1]
                c['spilled'] += cstats[2]
                c['records'] += cstats[3]
                c['bytes_used'] = max(c['bytes_used'], cstats[4])
            if event is not None:
                import torch
                cur = torch.cuda.current_stream(stream.device)
                cur.wait_event(event)
                for t in out.values():          # allocated on the copy stream, consumed (and later freed) on this one
                    t.record_stream(cur)
            return out
        self.close()
        if item[0] == "error":
            raise item[1]
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
