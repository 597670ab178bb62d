"""The host half of the device input pipeline without a GPU: input_pipeline.pack_batch plans a batch for every arm
(jpeg_decode='device', + jpeg_entropy='device', each with and without cache='device', eval and train), the plan is executed
here with NumPy copies and the host statements of the three kernels it names (ds_jpeg_entropy_decode_segments_host,
ds_jpeg_reconstruct_host, ds_ragged_gather_host), the status words go through input_pipeline.flagged_fallback, and what
arrives in the ragged buffer and the descriptor table must be pack_ragged over PIL's crops, byte for byte.  The records are
the smallest at which the chroma edge, the padding blocks and the 4-, 8- and 16-element alignments can go wrong, plus one
restart-marked stream that the segment decoder flags and PIL decodes.  The device tests (tests/test_input_pipeline_*_gpu.py,
tests/test_jpeg_entropy_gpu.py, tests/test_input_cache_gpu.py) run the same plans through the kernels."""
import functools
import io

import numpy as np
import pytest
import torch
from PIL import Image

from test_jpeg_cpu import encode, pixels
from test_jpeg_restart_cpu import quantiser_streams
from tumblr_emotions_amd import input_pipeline as P
from tumblr_emotions_amd import ops
from tumblr_emotions_amd.datasets import dataset_utils as du

SIZES = ((1, 1), (7, 5), (17, 33), (75, 100), (48, 64), (16, 16))          # (height, width)
OUT, SEED, ARENA = 24, 7, 40000
ARMS = {"jpeg": dict(jpeg=True), "entropy": dict(jpeg=True, entropy=True)}


def _png(a):
    bio = io.BytesIO()
    Image.fromarray(a).save(bio, "PNG")
    return bio.getvalue()


@functools.lru_cache(None)
def records():
    """[(kind, TFRecord payload)]: every size as a baseline JPEG (4:4:4, 4:2:2, 4:2:0 in turn), a 4:2:0 JPEG with one
    restart interval per MCU row, a PNG and a progressive JPEG; and the stream the segment decoder flags."""
    images = []
    for i, (h, w) in enumerate(SIZES):
        a = pixels(h, w, "noise", seed=i)
        images += [("baseline", encode(a, i % 3, 90), h, w), ("restart", encode(a, 2, 90, restart_marker_rows=1), h, w),
                   ("png", _png(a), h, w), ("progressive", encode(a, 2, 90, progressive=True), h, w)]
    images.append(("flagged", quantiser_streams(2)[255], 64, 64))
    rng = np.random.RandomState(1)
    return [(kind, du.image_to_tfexample_with_text(data, b'png' if kind == "png" else b'jpg', h, w,
                                                   rng.randint(0, 50, size=9).tolist(), 9, i % 5, i, i % 7))
            for i, (kind, data, h, w) in enumerate(images)]


@functools.lru_cache(None)
def reference(train, pass_no, kinds=None):
    """pack_ragged over decode_record's PIL crops of the records (of `kinds` only), in the order of slots(): (ragged bytes,
    descriptor table, bytes used)."""
    recs = [r for k, r in records() if kinds is None or k in kinds]
    crops = [P.decode_record(r, (SEED, pass_no, i) if train else None)[0] for i, r in enumerate(recs)]
    order = slots(len(recs))
    params = None
    if train:
        crops, params = [c for c, _ in crops], [p for _, p in crops]
        params = [params[j] for j in order]
    buf, desc, used = P.pack_ragged([crops[j] for j in order], OUT, OUT, params=params)
    return buf[:used], desc, used


def slots(n):
    return np.random.RandomState(3).permutation(n)             # output slot -> record of the pass: the batch permutation


def plan_batch(cfg, st, cache, pool, recs, pass_no):
    """One batch the way the feeder makes it: submit what is not resident, take the items in stream order, plan them in
    slot order."""
    decode = P.decode_record_jpeg_scan if cfg.entropy else P.decode_record_jpeg if cfg.jpeg else P.decode_record
    whole = cfg.train and cache is not None
    pending = []
    for idx, rec in enumerate(recs):
        slot = None
        if cache is None or (0, idx) not in cache.entries:
            slot = pool.submit(decode, rec, (SEED, pass_no, idx) if cfg.train and cache is None else None, whole)
        pending.append((slot, pass_no, idx, (0, idx)))
    items = [P._next_item(e, cfg, cache)[0] for e in pending]
    return P.pack_batch([items[j] for j in slots(len(recs))], OUT, OUT, st, cache is not None), whole


def execute(plan, st, cache, whole):
    """The device half of the feeder with NumPy copies and the kernels' host statements.  Returns (ragged buffer, the plan
    as flagged_fallback amended it, the status words)."""
    staged, ragged = st.bytes.numpy(), np.zeros(plan.used, np.uint8)
    arena = cache.arena.numpy() if cache is not None else None
    spill = st.spill_dev.numpy() if st.spill_dev is not None else None
    bufs = (arena, spill, ragged)

    def upload(copies):
        for dst, doff, soff, size in copies:
            bufs[dst][doff:doff + size] = staged[soff:soff + size]

    upload(plan.copies)
    coef = np.zeros(plan.ncoef, np.int16)
    for off, size in plan.coef_copies:
        coef[off:off + size] = st.coef.numpy()[off:off + size]
    status = np.zeros(0, np.int32)
    if plan.scans:
        status = ops.jpeg_entropy_decode_segments_host(st.scan.numpy()[:plan.nscan], st.sdesc_np[:len(plan.scans)],
                                                       st.segs_np[:plan.nseg], coef)
        issued = len(plan.copies)
        plan = P.flagged_fallback(plan, st, np.nonzero(status)[0], whole)
        upload(plan.copies[issued:])
    for dst, base, end, first, n in plan.groups:
        ops.jpeg_reconstruct_host(coef, st.jdesc_np[first:first + n], bufs[dst][base:end])
    if plan.gather:
        ops.ragged_gather_host(arena, spill, st.gdesc_np[:plan.gather], ragged)
    return ragged, plan, status


def check(cfg, st, plan, ragged, want):
    buf, desc, used = want
    assert plan.used == used
    assert np.array_equal(ragged, buf)
    assert st.desc_np[:cfg.batch_size].tobytes() == desc.tobytes()


def setup(train, arm, cache_bytes=None, n=None):
    cfg = P._Config(n or len(records()), OUT, OUT, torch.device("cpu"), train=train, seed=SEED, cache_bytes=cache_bytes, **arm)
    st = P._Staging(cfg, 9)
    st.bytes.zero_()            # staging memory is uninitialised and a ragged slot is copied with its padding: compare that too
    return cfg, st


@pytest.mark.parametrize("train", [False, True], ids=["eval", "train"])
@pytest.mark.parametrize("arm", sorted(ARMS))
def test_plan_reproduces_pack_ragged_over_pil_crops(arm, train):
    cfg, st = setup(train, ARMS[arm])
    recs = [r for _, r in records()]
    pool = P.OrderedPool(2)
    try:
        plan, whole = plan_batch(cfg, st, None, pool, recs, 0)
    finally:
        pool.close()
    kinds = [records()[j][0] for j in slots(len(recs))]
    on_device = sum(k in ("restart", "flagged") for k in kinds) if arm == "entropy" else 0
    assert len(plan.scans) == on_device and plan.gather == 0 and plan.stats is None
    assert plan.arrays == sum(k in ("png", "progressive") for k in kinds) + (arm == "jpeg")     # the host decoder leaves the flagged stream to PIL
    assert [g[0] for g in plan.groups] == [P._RAGGED] and plan.groups[0][1:3] == (0, plan.used)
    ragged, done, status = execute(plan, st, None, whole)
    assert done.flagged == (arm == "entropy") and int((status != 0).sum()) == done.flagged
    assert sum(g[4] for g in done.groups) == sum(g[4] for g in plan.groups) - done.flagged
    check(cfg, st, done, ragged, reference(train, 0))


@pytest.mark.parametrize("train", [False, True], ids=["eval", "train"])
@pytest.mark.parametrize("arm", sorted(ARMS))
def test_plan_with_the_cache_over_two_passes(arm, train):
    cfg, st = setup(train, ARMS[arm], cache_bytes=ARENA)
    cache = P._Cache(ARENA, cfg.device)
    recs = [r for _, r in records()]
    pool = P.OrderedPool(2)
    try:
        for pass_no in range(2):
            plan, whole = plan_batch(cfg, st, cache, pool, recs, pass_no)
            s = plan.stats
            assert plan.gather == len(recs) and s.hits + s.misses == len(recs) and s.records + s.spilled == s.misses
            if pass_no == 0:
                assert s.hits == 0 and s.records > 0 and s.spilled > 0 and 0 < s.bytes_used <= ARENA
                resident = s.records
            else:                                  # what found room is served from the arena; what spilled is decoded again
                assert s.hits == resident and s.misses == s.spilled == len(recs) - resident
                assert all(g[0] == P._SPILL for g in plan.groups) and all(c[0] == P._SPILL for c in plan.copies)
            ragged, done, _ = execute(plan, st, cache, whole)
            check(cfg, st, done, ragged, reference(train, pass_no))
    finally:
        pool.close()
    assert len(cache.entries) == resident and cache.full


@pytest.mark.parametrize("train", [False, True], ids=["eval", "train"])
def test_a_batch_of_arrays_is_one_copy(train):
    """The PIL arm through the common packer: every item an array, every destination the ragged buffer."""
    recs = [r for k, r in records() if k == "png"]
    cfg, st = setup(train, {}, n=len(recs))
    pool = P.OrderedPool(2)
    try:
        plan, whole = plan_batch(cfg, st, None, pool, recs, 0)
    finally:
        pool.close()
    assert plan.copies == [(P._RAGGED, 0, 0, plan.used)] and plan.groups == [] and plan.arrays == len(recs)
    assert plan.scans == [] and plan.coef_copies == [] and plan.gather == 0
    ragged, done, _ = execute(plan, st, None, whole)
    assert done is plan
    check(cfg, st, plan, ragged, reference(train, 0, ("png",)))
