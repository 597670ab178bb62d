"""cache='device' without a GPU: ds_ragged_gather_host -- the CPU statement of the kernel, the shared lines of
csrc/gather_common.h -- against NumPy slicing with guard bytes; ops.check_gather_descs; the loader's ordering and its
pass plan; and the same host code in a stand-alone sanitised program (tests/gather_host_driver.cpp).  Nothing loaded into
Python is sanitised.  tests/test_input_cache_gpu.py runs the same grid through the kernel and the loader on the device."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import gather_cases as G
from tumblr_emotions_amd import _lib, ops
from tumblr_emotions_amd import input_pipeline as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_host_statement_equals_numpy_slicing_and_writes_nothing_else():
    cases = G.cases()
    assert len(cases) > 200
    assert {int(c.desc.size) for c in cases} == {1, 7}
    assert any(c.spill is not None and (c.desc["src"] == 0).any() and (c.desc["src"] == 1).any() for c in cases)
    assert {int(w) * 3 % 16 for c in cases for w in c.desc["width"]} >= {3 * w % 16 for w in range(1, 10)}
    assert {int(x) % 4 for c in cases for x in c.desc["x0"] * 3} == {0, 1, 2, 3}
    for i, c in enumerate(cases):
        got = G.run_host(c)
        assert np.array_equal(got, c.want), (i, c.desc)      # the windows, and the guards and the gaps untouched


def _one(**kw):
    d = np.zeros(1, ops.gather_desc_dtype())
    d[0] = (0, 0, 0, 15, 0, 0, 2, 5)                           # a 2 x 5 window of a 5-pixel-wide image at byte 0
    for k, v in kw.items():
        d[k] = v
    return d


@pytest.mark.parametrize("fault, kw", [
    ("src must be", dict(src=2)),
    ("leaves its source", dict(x0=1)),                          # the window leaves its row
    ("leaves its source", dict(y0=3)),                          # ... its buffer (arena of 60 bytes)
    ("leaves its source", dict(src=1)),                         # a spill buffer that is not there
    ("outside the output", dict(out_offset=8)),
    ("multiple of 4", dict(out_offset=2)),
])
def test_descriptor_faults_raise_and_the_host_statement_leaves_the_image_alone(fault, kw):
    desc = _one(**kw)
    with pytest.raises(ValueError, match=fault):
        ops.check_gather_descs(desc, 60, 0, 32)
    arena, out = np.full(60, 9, np.uint8), G.pattern(32)
    rc = _lib.load().ds_ragged_gather_host(C.c_void_p(arena.ctypes.data), 60, None, 0, C.c_void_p(desc.ctypes.data), 1,
                                           C.c_void_p(out.ctypes.data), 32)
    assert rc == 0 and np.array_equal(out, G.pattern(32))
    ops.check_gather_descs(_one(), 60, 0, 32)


def test_overlapping_windows_and_bad_arguments():
    two = np.concatenate([_one(), _one(out_offset=28)])
    with pytest.raises(ValueError, match="overlap"):
        ops.check_gather_descs(two, 60, 0, 64)
    ops.check_gather_descs(np.concatenate([_one(), _one(out_offset=32)]), 60, 0, 64)
    with pytest.raises(ValueError, match="gather_desc_dtype"):
        ops.check_gather_descs(np.zeros(1, ops.preprocess_desc_dtype()), 60, 0, 64)
    lib, d, a = _lib.load(), _one(), np.zeros(60, np.uint8)
    p = lambda x: C.c_void_p(x.ctypes.data)
    assert lib.ds_ragged_gather_host(None, 60, None, 0, p(d), 1, p(a), 32) == -1           # DS_ERR_ARG
    assert lib.ds_ragged_gather_host(p(a), 60, None, 0, p(d), 0, p(a), 32) == -1
    assert lib.ds_ragged_gather_host(p(a), -1, None, 0, p(d), 1, p(a), 32) == -1
    assert lib.ds_ragged_gather(None, 60, None, 0, None, 1, None, 32, None) == -1 and b"ds_ragged_gather" in lib.ds_last_error()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.ragged_gather(torch.zeros(60, dtype=torch.uint8), None, d, torch.zeros(32, dtype=torch.uint8))


def test_a_bad_image_is_skipped_and_its_neighbours_are_copied():
    c = [c for c in G.cases() if c.desc.size == 7][0]
    desc = c.desc.copy()
    desc["src_offset"][3] = max(c.arena.size, 0 if c.spill is None else c.spill.size)       # past ops' check: the library directly
    big = c.guarded()
    out = big[G.GUARD:G.GUARD + c.nout]
    rc = _lib.load().ds_ragged_gather_host(C.c_void_p(c.arena.ctypes.data), c.arena.size,
                                           None if c.spill is None else C.c_void_p(c.spill.ctypes.data),
                                           0 if c.spill is None else c.spill.size, C.c_void_p(desc.ctypes.data), 7,
                                           C.c_void_p(out.ctypes.data), c.nout)
    want = c.want.copy()
    at, n = G.GUARD + int(desc["out_offset"][3]), int(desc["height"][3]) * int(desc["width"][3]) * 3
    want[at:at + n] = G.pattern(want.size)[at:at + n]
    assert rc == 0 and np.array_equal(big, want)


# ---- the loader's bookkeeping ------------------------------------------------------------------------------------------------------
def _text_dataset(root):
    from test_datasets_cpu import _make_dataset
    from tumblr_emotions_amd.datasets import convert_to_dataset as cd
    os.makedirs(root)
    _make_dataset(root, n_train=11, n_valid=3)
    return cd.get_split_with_text("train", root)


def test_the_switch_keeps_the_host_generators_order_without_a_device(tmp_path):
    """decode_images=False: cache='device' is accepted and does nothing, so this pins the RandomState order alone --
    three shuffled passes of 11 records in two shards at batch 4."""
    from tumblr_emotions_amd.image_model.im_model import load_batch_with_text
    ds = _text_dataset(str(tmp_path / "d"))
    kw = dict(batch_size=4, shuffle=True, device="cpu", seed=5, decode_images=False, max_token_id=100, num_classes=3)
    host = load_batch_with_text(ds, pipeline='host', **kw)
    with P.DeviceLoader(ds, workers=3, cache='device', cache_bytes=1 << 20, **kw) as dev:
        for i in range(3 * 11 // 4 + 1):
            a, b = next(host), next(dev)
            assert set(a) == set(b) == {"texts", "seq_lens", "labels", "post_ids", "days"}
            assert all(torch.equal(a[k], b[k]) for k in a), i
        assert dev.cache == 'device' and dev.cache_stats() == dict(hits=0, misses=0, spilled=0, bytes_used=0, bytes_capacity=0, records=0)
    host.close()


def test_the_switch_is_refused_where_it_cannot_work(tmp_path):
    from tumblr_emotions_amd.image_model.im_model import load_batch_with_text
    from tumblr_emotions_amd.training import SyntheticInput
    ds = _text_dataset(str(tmp_path / "d"))
    with pytest.raises(ValueError, match="pipeline='device'"):
        load_batch_with_text(ds, pipeline='host', cache='device', cache_bytes=1 << 20)
    with pytest.raises(ValueError, match="cache_bytes"):
        load_batch_with_text(ds, pipeline='device', device="cpu", decode_images=False, cache='device')
    with pytest.raises(ValueError, match="cache_bytes"):
        P.DeviceLoader(ds, device="cpu", decode_images=False, cache='device', cache_bytes=0)
    with pytest.raises(ValueError, match="cache must be"):
        P.DeviceLoader(ds, device="cpu", decode_images=False, cache='host')
    with pytest.raises(ValueError, match="CUDA/HIP device"):
        P.DeviceLoader(ds, device="cpu", cache='device', cache_bytes=1 << 20)
    init = lambda cfg: SyntheticInput()._init_input(dict(cfg, synthetic=True), 50, 10, 3, True, "cpu")
    with pytest.raises(ValueError, match="input_cache"):
        init({"input_cache": "device", "input_cache_gb": 1.0, "input_pipeline": "device"})            # synthetic
    with pytest.raises(ValueError, match="input_cache"):
        SyntheticInput()._init_input({"input_cache": "device", "input_cache_gb": 1.0, "dataset_dir": str(tmp_path / "d")},
                                     50, 10, 3, True, "cpu")                                         # the host pipeline
    with pytest.raises(ValueError, match="input_cache_gb"):
        SyntheticInput()._init_input({"input_cache": "device", "input_pipeline": "device", "dataset_dir": str(tmp_path / "d")},
                                     50, 10, 3, True, "cpu")
    with pytest.raises(ValueError, match="input_cache"):
        init({"input_cache": "hbm"})
    init({"input_cache": "none"})


def test_pass_plan_names_exactly_the_sources_that_hold_a_miss():
    counts = [6, 5, 4]                                       # three source files
    everything = {(s, r) for s in range(3) for r in range(counts[s])}
    for world, rank in ((1, 0), (2, 0), (2, 1)):
        for order in ((0, 1, 2), (2, 0, 1)):
            assert P.sources_to_open(counts, order, rank, world, everything) == []             # a fully cached pass opens nothing
            assert P.sources_to_open(counts, order, rank, world, set()) == list(order)
    # world = 2, shuffled: the records of a rank are every other one of the SHUFFLED order, so what it needs moves with the pass
    order = (2, 0, 1)                                        # global indices: source 2 -> 0..3, source 0 -> 4..9, source 1 -> 10..14
    mine = lambda rank: {(s, r) for s, first in ((2, 0), (0, 4), (1, 10)) for r in range(counts[s]) if (first + r) % 2 == rank}
    assert P.sources_to_open(counts, order, 0, 2, mine(0)) == [] and P.sources_to_open(counts, order, 1, 2, mine(1)) == []
    assert P.sources_to_open(counts, order, 1, 2, mine(0)) == [2, 0, 1]
    assert P.sources_to_open(counts, order, 0, 2, mine(0) - {(0, 2)}) == [0]                   # index 6: rank 0's
    assert P.sources_to_open(counts, order, 1, 2, everything - {(0, 2)}) == []                 # ... and not rank 1's
    assert P.sources_to_open(counts, order, 1, 2, everything - {(1, 1), (2, 1)}) == [2, 1]     # indices 11 and 1
    assert P.sources_to_open(counts, (0, 1, 2), 0, 2, mine(0)) != []                           # another pass order, other records
    # a source of unknown size is opened, and so is every source behind it: their global indices are not known yet
    assert P.sources_to_open([6, None, 4], (0, 1, 2), 0, 1, everything) == [1, 2]
    assert P.source_has_miss(1, 5, 10, 1, 2, everything - {(1, 2)}) is False and P.source_has_miss(1, 5, 10, 0, 2, everything - {(1, 2)}) is True


def test_cached_record_stream_opens_only_what_the_plan_names(tmp_path, monkeypatch):
    """The stream itself, with a plain index in place of the arena: the records, their order and the draws of the host
    generator's stream, and no read of a source whose records of this rank are all resident."""
    from tumblr_emotions_amd.datasets import tfrecord
    ds = _text_dataset(str(tmp_path / "d"))
    opened = []
    real = tfrecord.read_records
    monkeypatch.setattr(tfrecord, "read_records", lambda path: (opened.append(path), real(path))[1])

    class Index:
        entries, counts = {}, {}

    for world, rank in ((1, 0), (2, 1)):
        Index.entries, Index.counts = {}, {}
        rng_a, rng_b = np.random.RandomState(5), np.random.RandomState(5)
        plain = P._record_stream(ds, True, rng_a, rank, world, True)
        cached = P._record_stream(ds, True, rng_b, rank, world, True, Index)
        opens = []
        for pass_no in range(4):
            del opened[:]
            while True:
                a, b = next(plain), next(cached)
                if a is P._EPOCH:
                    assert b is P._EPOCH
                    break
                assert a[:3] == b[:3] and a[3] is not None
                if b[3] is None:
                    assert b[2] in Index.entries
                else:
                    assert bytes(a[3]) == bytes(b[3])
                    Index.entries[b[2]] = True
            opens.append(len(opened) - 2)                     # the plain stream opens both files on every pass
        assert opens[0] == 2 and (opens[1:] == [0, 0, 0] if world == 1 else opens[-1] <= 2)
        assert sum(Index.counts.values()) == 11


# ---- the same host code, sanitised, in a program of its own ------------------------------------------------------------------------
def _compiler():
    for name in (os.environ.get("CXX"), "c++", "g++", "clang++"):
        if name and shutil.which(name):
            return shutil.which(name)
    pytest.fail("no host C++ compiler (c++ / g++ / clang++) to build the sanitised driver with")


def test_sanitised_host_statement_survives_the_grid_and_random_descriptors(tmp_path):
    exe = str(tmp_path / "gather_host_driver")
    cxx = _compiler()
    static = []                                   # the sanitizer runtime linked INTO the program: nothing has to be preloaded
    for flags in (["-static-libasan", "-static-libubsan"], ["-static-libsan"]):           # gcc's spelling, clang's
        probe = subprocess.run([cxx, *flags, "-fsanitize=address,undefined", "-x", "c++", "-", "-o", str(tmp_path / "probe")],
                               input="int main() { return 0; }\n", capture_output=True, text=True)
        if probe.returncode == 0:
            static = flags
            break
    build = subprocess.run([cxx, "-std=c++17", *static, "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-fno-omit-frame-pointer", "-I", os.path.join(ROOT, "include"),
                            "-I", os.path.join(ROOT, "tumblr_emotions_amd", "csrc"),
                            os.path.join(ROOT, "tests", "gather_host_driver.cpp"),
                            os.path.join(ROOT, "tumblr_emotions_amd", "csrc", "gather_host.cpp"), "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0")
    run = subprocess.run([exe, "400", "20261018"], capture_output=True, text=True, env=env, timeout=300)
    assert run.returncode == 0, (run.returncode, run.stdout[-2000:], run.stderr[-6000:])
    assert "ERROR" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-6000:]
    grid, copied, skipped = [int(x) for x in run.stdout.split()[1::2]]
    assert grid > 300 and copied > 0 and skipped > 0 and copied + skipped == 400
