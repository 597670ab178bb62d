#!/usr/bin/env python
"""The input pipelines, measured on one dataset in one session ("Real-data input pipeline").

    input_pipeline_bench.py [--out DIR] [--images 4096] [--seconds 5] [--json FILE] [parts ...]

Writes a seeded dataset of 500 x 375 JPEGs (quality 90, smooth content) under DIR, then, per part:
  loader   loader-only images/s at batch 256: the host pipeline against the device pipeline at 1, 2, 4, 8, 16 workers,
           alternating host and device windows of >= `seconds` each, every loader after a warm-up epoch
  train    joint fp32 training samples/s at batch 256 from that dataset, host against device at 8 workers, and the same
           step on a resident batch (the step time the kernel's share is taken of)
  kernel   ds_preprocess_eval at B = 256 (device events), the bytes it must move; run this part alone under
           `rocprofv3 --kernel-trace --stats` for the profiler's figure and pass the stats file back with --kernel-stats
  kernel_train   ds_preprocess_train at B = 256 on crops drawn by sample_train_params from 375 x 500 sources, beside
           ds_preprocess_eval on the SAME packed crops (same bytes in and out: the eval kernel is the baseline); the part to run
           under `rocprofv3 --kernel-trace --stats`
  augment  device pipeline at 8 workers, alternating windows without and with is_training=True; the cost of
           record_rng + sample_train_params per image on one thread (ordinary and 100-attempt sizes)
  jpeg     the third arm: device pipeline + jpeg_decode='device' beside the device pipeline decoding with PIL (the yardstick: the
           parent's path, same worker count, same session) and the host pipeline, alternating windows at 1, 2, 4, 8, 16
           workers; ds_jpeg_reconstruct at B = 256 by device events, the coefficient bytes per batch against the pixel bytes
           they replace, the fallback count, and the kernel's share of the training step (--step-ms, default the 13.06 ms
           of bench.py's resident-batch step at 19.6k samples/s) against the 2 % budget of DESIGN.md 7.2.  All three loaders
           of a worker count stay alive through its windows: at every switch the idle arms refill their prefetch queues
           on their own worker pools, which overlaps the first batches of the measured arm -- read the rates with that in mind.
           The fourth arm: the same images rewritten by add_restart_markers (one restart interval per MCU row) read with
           jpeg_entropy='device', beside ITS yardstick -- jpeg_decode='device' alone on the same restart-marked files --
           in the same alternation; the growth of the files, and ds_jpeg_entropy_decode_device at B = 256 by device events
           with the bytes it reads against the coefficient bytes whose upload it replaces (--workers picks the worker counts)
  cache    the decoded-image cache (cache='device', --cache-gb of arena) on the restart-marked files with jpeg_entropy='device',
           eval chain and is_training=True, at the worker counts of --workers: pass 0 (a fresh loader's first epoch, arena
           writes included) beside the first epoch of a fresh loader of its yardstick arm, then alternating windows of the
           steady state (passes >= 1: every record a hit) and of the parent's three arms (device + PIL, jpeg_decode='device',
           + jpeg_entropy='device' on the restart files); the feeder's host time per cached batch; ds_ragged_gather at
           B = 256 by device events, launch by launch, on the eval windows and on sampled train windows, against the 2 %
           budget of DESIGN.md 7.2.  Writes profiles/input_pipeline_cache.json as well.
One JSON line per measurement on stdout; everything is merged into FILE (default DIR/input_pipeline.json)."""
import argparse
import concurrent.futures
import csv
import io
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

B, H, W, OUT = 256, 375, 500, 224
V, D, RNN = 10000, 300, 512


def make_dataset(root, n, shards=8, seed=0):
    from PIL import Image
    from tumblr_emotions_amd.datasets import convert_to_dataset as cd
    from tumblr_emotions_amd.datasets import dataset_utils as du
    from tumblr_emotions_amd.datasets import tfrecord as T
    if os.path.exists(os.path.join(root, "photos", cd._TRAIN_VALID_FILENAME)):
        return cd.get_split_with_text("train", root)
    os.makedirs(os.path.join(root, "photos"))
    os.makedirs(os.path.join(root, "tfrecords"))
    du.write_label_file({i: "emotion%d" % i for i in range(15)}, root, "photos")
    with open(os.path.join(root, "photos", cd._TRAIN_VALID_FILENAME), "w") as f:
        f.write("train:%d\nvalidation:0\n" % n)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)

    def one(i):
        r = np.random.RandomState(seed * 100003 + i)
        a, b, c, d = r.uniform(20, 90, size=4)
        p = r.uniform(0, 6.28, size=3)
        img = np.stack([128 + 110 * np.sin(yy / a + p[0]) * np.cos(xx / b), 128 + 110 * np.sin((xx + yy) / c + p[1]),
                        128 + 110 * np.cos(xx / d + p[2])], axis=2) + r.normal(0, 3, size=(H, W, 3))
        buf = io.BytesIO()
        Image.fromarray(np.clip(img, 0, 255).astype(np.uint8)).save(buf, format="JPEG", quality=90)
        text = r.randint(0, V, size=50).tolist()
        return du.image_to_tfexample_with_text(buf.getvalue(), b'jpg', H, W, text, int(r.randint(5, 51)), int(r.randint(15)),
                                               i, i % 7)

    with concurrent.futures.ThreadPoolExecutor(16) as ex:
        recs = list(ex.map(one, range(n)))
    for s in range(shards):
        T.write_records(cd.dataset_filename(root, "tfrecords", "train", s, shards), recs[s::shards])
    return cd.get_split_with_text("train", root)


def restart_dataset(ds, root):
    """The dataset's images with one restart interval per MCU row (add_restart_markers, written once beside the original
    shards) and what the transcode cost in file size."""
    from tumblr_emotions_amd.datasets import convert_to_dataset as cd
    if not os.path.isdir(os.path.join(root, "tfrecords_rst")):
        done = cd.add_restart_markers(root)
        assert done == (ds.num_samples, 0), done
    size = lambda sub: sum(os.path.getsize(os.path.join(root, sub, f)) for f in os.listdir(os.path.join(root, sub)))
    a, b = size("tfrecords"), size("tfrecords_rst")
    growth = dict(images=ds.num_samples, bytes_before=a, bytes_after=b, bytes_per_image=round((b - a) / ds.num_samples, 1),
                  relative=round((b - a) / a, 5))
    return cd.get_split_with_text("train", root, tfrecords_subdir="tfrecords_rst"), growth


def emit(results, **kw):
    results.append(kw)
    print(json.dumps(kw), flush=True)


def _window(it, seconds):
    import torch
    torch.cuda.synchronize()
    t0, n = time.perf_counter(), 0
    while time.perf_counter() - t0 < seconds:
        b = next(it)
        n += int(b["labels"].shape[0])
    torch.cuda.synchronize()               # the last batch's preprocessing has finished, too
    return n / (time.perf_counter() - t0)


def part_loader(ds, args, results):
    from tumblr_emotions_amd.image_model.im_model import load_batch_with_text
    kw = dict(batch_size=B, height=OUT, width=OUT, max_token_id=V, num_classes=15)
    epoch = ds.num_samples // B
    host = load_batch_with_text(ds, pipeline='host', **kw)
    for _ in range(epoch):
        next(host)
    for workers in (1, 2, 4, 8, 16):
        h = _window(host, args.seconds)
        dev = load_batch_with_text(ds, pipeline='device', workers=workers, **kw)
        for _ in range(epoch):
            next(dev)
        d = _window(dev, args.seconds)
        dev.close()
        emit(results, what="loader", workers=workers, host_images_per_s=round(h, 1), device_images_per_s=round(d, 1),
             ratio=round(d / h, 2))


def part_train(ds, args, results):
    import torch
    from tumblr_emotions_amd.image_model.im_model import load_batch_with_text
    from tumblr_emotions_amd.net import SentimentNet
    net = SentimentNet(mode="joint", nb_emotions=15, im_features_size=256, rnn_size=RNN, fc_size=512, vocab_size=V,
                       embedding_dim=D, post_size=50, dropout_keep_prob=0.8)
    net.initialize(seed=1)
    kw = dict(batch_size=B, height=OUT, width=OUT, max_token_id=V, num_classes=15)

    def run(it, seconds, warm):
        for _ in range(warm):
            net.train_step(next(it), 1e-3)
        torch.cuda.synchronize()
        t0, n = time.perf_counter(), 0
        while time.perf_counter() - t0 < seconds:
            net.train_step(next(it), 1e-3)
            n += B
        torch.cuda.synchronize()
        return n / (time.perf_counter() - t0)

    dev = load_batch_with_text(ds, pipeline='device', workers=8, **kw)
    resident = next(dev)
    for _ in range(10):
        net.train_step(resident, 1e-3)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(50):
        net.train_step(resident, 1e-3)
    torch.cuda.synchronize()
    step_ms = (time.perf_counter() - t0) / 50 * 1e3
    emit(results, what="step_resident_batch", ms=round(step_ms, 3), samples_per_s=round(B / step_ms * 1e3, 1))
    d = run(dev, args.seconds, ds.num_samples // B)
    dev.close()
    host = load_batch_with_text(ds, pipeline='host', **kw)
    h = run(host, args.seconds, 2)
    emit(results, what="train_joint_fp32", batch=B, host_samples_per_s=round(h, 1), device8_samples_per_s=round(d, 1),
         ratio=round(d / h, 2))


def part_kernel(ds, args, results):
    import torch
    from tumblr_emotions_amd import input_pipeline as P
    from tumblr_emotions_amd import ops
    rng = np.random.RandomState(0)
    y0, x0, ch, cw = P.crop_box(H, W)
    images = [rng.randint(0, 256, size=(ch, cw, 3)).astype(np.uint8) for _ in range(B)]
    buf, desc, used = P.pack_ragged(images, OUT, OUT)
    dbytes = torch.from_numpy(buf[:used]).cuda()
    ddesc = torch.from_numpy(desc.view(np.uint8)).cuda()
    out = torch.empty(B, OUT, OUT, 3, device="cuda")
    for _ in range(5):
        ops.preprocess_eval(dbytes, desc, OUT, OUT, desc_dev=ddesc, out=out)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(50):
        ops.preprocess_eval(dbytes, desc, OUT, OUT, desc_dev=ddesc, out=out)
    e1.record()
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) / 50 * 1e3
    moved = used + out.numel() * 4
    emit(results, what="ds_preprocess_eval", B=B, crop="%dx%d" % (ch, cw), read_bytes=used, write_bytes=out.numel() * 4,
         us_events=round(us, 1), tb_per_s=round(moved / us / 1e6, 3))


def part_kernel_train(ds, args, results):
    import torch
    from tumblr_emotions_amd import input_pipeline as P
    from tumblr_emotions_amd import ops
    from tumblr_emotions_amd.preprocessing import inception_preprocessing as ip
    rng = np.random.RandomState(0)
    params = [ip.sample_train_params(H, W, ip.record_rng(0, 0, i)) for i in range(B)]
    images = [rng.randint(0, 256, size=(p.crop_h, p.crop_w, 3)).astype(np.uint8) for p in params]
    buf, tdesc, used = P.pack_ragged(images, OUT, OUT, params=params)
    _, edesc, _ = P.pack_ragged(images, OUT, OUT)
    dbytes = torch.from_numpy(buf[:used]).cuda()
    out = torch.empty(B, OUT, OUT, 3, device="cuda")
    moved = used + out.numel() * 4
    for what, fn, desc in (("ds_preprocess_eval_on_train_crops", ops.preprocess_eval, edesc),
                           ("ds_preprocess_train", ops.preprocess_train, tdesc)):
        ddesc = torch.from_numpy(desc.view(np.uint8)).cuda()
        for _ in range(5):
            fn(dbytes, desc, OUT, OUT, desc_dev=ddesc, out=out)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(50):
            fn(dbytes, desc, OUT, OUT, desc_dev=ddesc, out=out)
        e1.record()
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) / 50 * 1e3
        emit(results, what=what, B=B, source="%dx%d" % (H, W), mean_crop_pixels=int(np.mean([im.size // 3 for im in images])),
             read_bytes=used, write_bytes=out.numel() * 4, us_events=round(us, 1), tb_per_s=round(moved / us / 1e6, 3))


def part_augment(ds, args, results):
    from tumblr_emotions_amd.image_model.im_model import load_batch_with_text
    from tumblr_emotions_amd.preprocessing import inception_preprocessing as ip
    for name, (h, w) in (("ordinary_375x500", (H, W)), ("fallback_50x1000", (50, 1000))):
        n = 20000 if name.startswith("ordinary") else 2000
        t0 = time.perf_counter()
        for i in range(n):
            ip.sample_train_params(h, w, ip.record_rng(0, 0, i))
        emit(results, what="sample_train_params", size=name, us_per_image=round((time.perf_counter() - t0) / n * 1e6, 1))
    kw = dict(batch_size=B, height=OUT, width=OUT, max_token_id=V, num_classes=15, pipeline='device', workers=8)
    epoch = ds.num_samples // B
    plain = load_batch_with_text(ds, **kw)
    aug = load_batch_with_text(ds, is_training=True, **kw)
    for it in (plain, aug):
        for _ in range(epoch):
            next(it)
    rates = {"eval": [], "augment": []}
    for _ in range(args.windows):
        rates["eval"].append(_window(plain, args.seconds))
        rates["augment"].append(_window(aug, args.seconds))
    plain.close()
    aug.close()
    e, a = rates["eval"], rates["augment"]
    emit(results, what="device_pipeline_augment", workers=8, windows=args.windows, seconds=args.seconds,
         eval_images_per_s=[round(x, 1) for x in e], augment_images_per_s=[round(x, 1) for x in a],
         eval_mean=round(float(np.mean(e)), 1), augment_mean=round(float(np.mean(a)), 1),
         eval_spread=round(float(max(e) - min(e)), 1), ratio=round(float(np.mean(a) / np.mean(e)), 3))


def part_jpeg(ds, args, results):
    import torch
    from tumblr_emotions_amd import input_pipeline as P
    from tumblr_emotions_amd import ops
    from tumblr_emotions_amd.datasets.tfrecord import read_records
    from tumblr_emotions_amd.image_model.im_model import load_batch_with_text
    kw = dict(batch_size=B, height=OUT, width=OUT, max_token_id=V, num_classes=15)
    epoch = ds.num_samples // B
    host = load_batch_with_text(ds, pipeline='host', **kw)
    for _ in range(2):
        next(host)
    ds_rst, growth = restart_dataset(ds, os.path.join(args.out, "dataset"))
    emit(results, what="restart_transcode_growth", **growth)
    for workers in [int(w) for w in args.workers.split(",")]:
        pil = load_batch_with_text(ds, pipeline='device', workers=workers, **kw)
        jpg = load_batch_with_text(ds, pipeline='device', workers=workers, jpeg_decode='device', **kw)
        rst = load_batch_with_text(ds_rst, pipeline='device', workers=workers, jpeg_decode='device', **kw)
        ent = load_batch_with_text(ds_rst, pipeline='device', workers=workers, jpeg_decode='device', jpeg_entropy='device', **kw)
        for it in (pil, jpg, rst, ent):
            for _ in range(epoch):
                next(it)
        rates = {"host": [], "pil": [], "jpeg": [], "jpeg_rst": [], "entropy": []}
        for _ in range(args.windows):
            rates["host"].append(_window(host, args.seconds))
            rates["pil"].append(_window(pil, args.seconds))
            rates["jpeg"].append(_window(jpg, args.seconds))
            rates["jpeg_rst"].append(_window(rst, args.seconds))
            rates["entropy"].append(_window(ent, args.seconds))
        fallbacks = jpg.jpeg_fallbacks
        r, e = rates["jpeg_rst"], rates["entropy"]
        emit(results, what="loader_jpeg_entropy", workers=workers, windows=args.windows, seconds=args.seconds,
             yardstick_jpeg_on_restart_files_windows=[round(x, 1) for x in r], device_entropy_windows=[round(x, 1) for x in e],
             yardstick_images_per_s=round(float(np.mean(r)), 1), device_entropy_images_per_s=round(float(np.mean(e)), 1),
             yardstick_spread=round(float(max(r) - min(r)), 1), gain=round(float(np.mean(e) - np.mean(r)), 1),
             ratio_entropy_over_yardstick=round(float(np.mean(e) / np.mean(r)), 3),
             beats_yardstick_by_more_than_its_spread=bool(np.mean(e) - np.mean(r) > max(r) - min(r)),
             device_entropy_images=ent.jpeg_device_entropy, fallbacks=ent.jpeg_fallbacks, yardstick_fallbacks=rst.jpeg_fallbacks)
        for it in (pil, jpg, rst, ent):
            it.close()
        m = {k: float(np.mean(v)) for k, v in rates.items()}
        emit(results, what="loader_jpeg", workers=workers, windows=args.windows, seconds=args.seconds,
             host_images_per_s=round(m["host"], 1), device_pil_images_per_s=round(m["pil"], 1),
             device_jpeg_images_per_s=round(m["jpeg"], 1), device_pil_windows=[round(x, 1) for x in rates["pil"]],
             device_jpeg_windows=[round(x, 1) for x in rates["jpeg"]], ratio_jpeg_over_pil=round(m["jpeg"] / m["pil"], 3),
             jpeg_fallbacks=fallbacks)
    # the kernel alone: one batch of the dataset's own records
    recs = []
    for rec in read_records(ds.data_sources[0]):
        recs.append(bytes(rec))
        if len(recs) == B:
            break
    cfg = P._Config(B, OUT, OUT, torch.device("cuda"), jpeg=True)
    pool = P.OrderedPool(8)
    pending = [(pool.submit(P.decode_record_jpeg, r), 0, i, None) for i, r in enumerate(recs)]
    items = [P._next_item(e, cfg)[0] for e in pending]
    pool.close()
    st = P._Staging(cfg, 50)
    plan = P.pack_batch(items, OUT, OUT, st)
    used, ncoef, nj = plan.used, plan.ncoef, sum(rows for _, _, _, _, rows in plan.groups)
    coef = st.coef[:ncoef].cuda()
    ddesc = st.jdesc.cuda()
    out = torch.empty(used, dtype=torch.uint8, device="cuda")
    scratch = torch.empty(ncoef, dtype=torch.uint8, device="cuda")
    for _ in range(5):
        ops.jpeg_reconstruct(coef, st.jdesc_np[:nj], out, scratch=scratch, desc_dev=ddesc)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(50):
        ops.jpeg_reconstruct(coef, st.jdesc_np[:nj], out, scratch=scratch, desc_dev=ddesc)
    e1.record()
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) / 50 * 1e3
    emit(results, what="ds_jpeg_reconstruct", B=B, device_decoded=nj, coef_bytes=2 * ncoef, pixel_bytes=used,
         coef_over_pixel_bytes=round(2 * ncoef / used, 3), us_events=round(us, 1), step_ms=args.step_ms,
         share_of_step=round(us / 1e3 / args.step_ms, 4), budget_share=0.02)
    # the entropy kernel alone: one batch of the restart-marked records
    recs = []
    for rec in read_records(ds_rst.data_sources[0]):
        recs.append(bytes(rec))
        if len(recs) == B:
            break
    items = [P.decode_record_jpeg_scan(r)[0] for r in recs]
    assert all(isinstance(it, P.JpegScan) for it in items)
    scan, images, segs, ncoef = ops.make_jpeg_scan_tables([(it.data, it.info, it.scan, it.cuts) for it in items])
    dscan, dimg, dseg = torch.from_numpy(scan).cuda(), torch.from_numpy(images.view(np.uint8)).cuda(), torch.from_numpy(segs.view(np.uint8)).cuda()
    coef = torch.empty(ncoef, dtype=torch.int16, device="cuda")
    status = torch.empty(B, dtype=torch.int32, device="cuda")
    run = lambda: ops.jpeg_entropy_decode_device(dscan, images, segs, coef, images_dev=dimg, segs_dev=dseg, status=status)
    for _ in range(3):
        run()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(20):
        run()
    e1.record()
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) / 20 * 1e3
    emit(results, what="ds_jpeg_entropy_decode_device", B=B, segments=int(segs.size), flagged=int((status != 0).sum()),
         scan_bytes=int(scan.size), table_bytes=int(images.nbytes + segs.nbytes), coef_bytes=2 * ncoef,
         upload_ratio=round(2 * ncoef / (scan.size + images.nbytes + segs.nbytes), 2), us_events=round(us, 1),
         images_per_s_kernel_alone=round(B / us * 1e6, 1), step_ms=args.step_ms, share_of_step=round(us / 1e3 / args.step_ms, 4))


def _first_epoch(make, epoch):
    """images/s of a fresh loader's first `epoch` batches, from its construction to the end of the last batch's kernels."""
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    it = make()
    for _ in range(epoch):
        next(it)
    torch.cuda.synchronize()
    return it, B * epoch / (time.perf_counter() - t0)


def part_cache(ds, args, results):
    import torch
    from tumblr_emotions_amd import input_pipeline as P
    from tumblr_emotions_amd import ops
    from tumblr_emotions_amd.image_model.im_model import load_batch_with_text
    from tumblr_emotions_amd.preprocessing.inception_preprocessing import record_rng, sample_train_params
    first = len(results)
    epoch = ds.num_samples // B
    ds_rst, _ = restart_dataset(ds, os.path.join(args.out, "dataset"))
    nbytes = int(args.cache_gb * 1e9)
    ent = dict(pipeline='device', jpeg_decode='device', jpeg_entropy='device')
    for train in (False, True):
        kw = dict(batch_size=B, height=OUT, width=OUT, max_token_id=V, num_classes=15, is_training=train)
        for workers in [int(w) for w in args.workers.split(",")]:
            pass0, yard0 = [], []
            for _ in range(args.windows):              # pass 0: fresh loaders, the cache arm and its yardstick in turn
                it, r = _first_epoch(lambda: load_batch_with_text(ds_rst, workers=workers, cache='device', cache_bytes=nbytes, **ent, **kw), epoch)
                pass0.append(r)
                it.close()
                it, r = _first_epoch(lambda: load_batch_with_text(ds_rst, workers=workers, **ent, **kw), epoch)
                yard0.append(r)
                it.close()
            arms = {"pil": load_batch_with_text(ds, pipeline='device', workers=workers, **kw),
                    "jpeg": load_batch_with_text(ds, pipeline='device', workers=workers, jpeg_decode='device', **kw),
                    "entropy": load_batch_with_text(ds_rst, workers=workers, **ent, **kw),
                    "cache": load_batch_with_text(ds_rst, workers=workers, cache='device', cache_bytes=nbytes, **ent, **kw)}
            for it in arms.values():
                for _ in range(epoch + 2):
                    next(it)
            rates = {k: [] for k in arms}
            for _ in range(args.windows):
                for k, it in arms.items():
                    rates[k].append(_window(it, args.seconds))
            stats = arms["cache"].cache_stats()
            for it in arms.values():
                it.close()
            best = max(("pil", "jpeg", "entropy"), key=lambda k: np.mean(rates[k]))
            y, c = rates[best], rates["cache"]
            emit(results, what="loader_cache", is_training=train, workers=workers, windows=args.windows, seconds=args.seconds,
                 cache_gb=args.cache_gb, pass0_windows=[round(x, 1) for x in pass0], pass0_yardstick_windows=[round(x, 1) for x in yard0],
                 pass0_images_per_s=round(float(np.mean(pass0)), 1), pass0_yardstick_images_per_s=round(float(np.mean(yard0)), 1),
                 steady_windows=[round(x, 1) for x in c], steady_images_per_s=round(float(np.mean(c)), 1),
                 **{"%s_windows" % k: [round(x, 1) for x in rates[k]] for k in ("pil", "jpeg", "entropy")},
                 best_yardstick=best, best_yardstick_images_per_s=round(float(np.mean(y)), 1),
                 best_yardstick_spread=round(float(max(y) - min(y)), 1), gain=round(float(np.mean(c) - np.mean(y)), 1),
                 beats_best_yardstick_by_more_than_its_spread=bool(np.mean(c) - np.mean(y) > max(y) - min(y)),
                 resident_step_samples_per_s=19400, passes_resident_step=bool(np.mean(c) > 19400), **stats)
    # where a cached batch's host time goes: the feeder's work for 256 hits, no device in the loop
    rng = np.random.RandomState(0)
    ch, cw = P.crop_box(H, W)[2:]
    for train in (False, True):
        st = P._Staging(P._Config(B, OUT, OUT, torch.device("cuda"), train=train, cache_bytes=1), 50)
        t0 = time.perf_counter()
        for rep in range(20):
            items = []
            for i in range(B):
                h, w = (H, W) if train else (ch, cw)
                p, box = None, (0, 0, h, w)
                if train:
                    p = sample_train_params(h, w, record_rng(0, rep, i))
                    box = (p.y0, p.x0, p.crop_h, p.crop_w)
                items.append(P._Item(i * (-(-h * w * 3 // 16) * 16), h, w, None, p, box))
            P.pack_batch(items, OUT, OUT, st, cached=True)
        emit(results, what="cache_feeder_host_time", is_training=train, B=B,
             ms_per_batch=round((time.perf_counter() - t0) / 20 * 1e3, 3))
    # the kernel alone
    for train in (False, True):
        h, w = (H, W) if train else (ch, cw)
        size = -(-h * w * 3 // 16) * 16
        arena = torch.from_numpy(rng.randint(0, 256, B * size).astype(np.uint8)).cuda()
        desc = np.zeros(B, ops.gather_desc_dtype())
        pos = 0
        for i in range(B):
            box = (0, 0, h, w)
            if train:
                p = sample_train_params(h, w, record_rng(0, 0, i))
                box = (p.y0, p.x0, p.crop_h, p.crop_w)
            desc[i] = (i * size, pos, 0, 3 * w, box[0], box[1], box[2], box[3])
            pos = -(-(pos + box[2] * box[3] * 3) // 4) * 4
        out = torch.empty(pos, dtype=torch.uint8, device="cuda")
        ddesc = torch.from_numpy(desc.view(np.uint8)).cuda()
        for _ in range(5):
            ops.ragged_gather(arena, None, desc, out, desc_dev=ddesc)
        times = []
        for _ in range(40):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ops.ragged_gather(arena, None, desc, out, desc_dev=ddesc)
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1) * 1e3)
        med = float(np.median(times))
        emit(results, what="ds_ragged_gather", windows="train" if train else "eval", B=B, bytes_in_and_out=2 * pos,
             us_median=round(med, 1), us_min=round(min(times), 1), us_max=round(max(times), 1),
             gb_per_s=round(2 * pos / med / 1e3, 1), step_ms=args.step_ms, share_of_step=round(med / 1e3 / args.step_ms, 4),
             budget_us=round(0.02 * args.step_ms * 1e3, 1), within_budget=bool(med <= 0.02 * args.step_ms * 1e3))
    prof = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "input_pipeline_cache.json")
    with open(prof, "w") as f:
        json.dump(results[first:], f, indent=1)


def kernel_stats(path, results):
    """Average duration of the preprocessing kernels from a rocprofv3 --kernel-trace --stats csv (Name, Calls, ..., AverageNs)."""
    with open(path) as f:
        for row in csv.DictReader(f):
            for k in ("preprocess_eval_kernel", "preprocess_train_kernel"):
                if k in row.get("Name", ""):
                    emit(results, what="ds_%s_rocprofv3" % k[:-len("_kernel")], calls=int(row["Calls"]),
                         us_average=round(float(row["AverageNs"]) / 1e3, 1))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="bench_outputs/input_pipeline")
    ap.add_argument("--images", type=int, default=4096)
    ap.add_argument("--seconds", type=float, default=5.0)
    ap.add_argument("--windows", type=int, default=4)
    ap.add_argument("--json", default=None)
    ap.add_argument("--step-ms", type=float, default=13.06)
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--workers", default="1,2,4,8,16", help="worker counts of the jpeg and cache parts")
    ap.add_argument("--cache-gb", type=float, default=3.0, help="arena of the cache part (4096 images of 500 x 375: 2.3 GB)")
    ap.add_argument("parts", nargs="*", default=["loader", "train", "kernel"])
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    path = args.json or os.path.join(args.out, "input_pipeline.json")
    results = json.load(open(path)) if os.path.exists(path) else []
    if args.kernel_stats:
        kernel_stats(args.kernel_stats, results)
    else:
        ds = make_dataset(os.path.join(args.out, "dataset"), args.images)
        for p in args.parts:
            {"loader": part_loader, "train": part_train, "kernel": part_kernel, "kernel_train": part_kernel_train,
             "augment": part_augment, "jpeg": part_jpeg, "cache": part_cache}[p](ds, args, results)
    with open(path, "w") as f:
        json.dump(results, f, indent=1)
