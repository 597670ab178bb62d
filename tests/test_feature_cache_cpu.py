"""The Mixed_5b feature cache without a GPU: ds_rows_gather_host -- the CPU statement of the kernel, the shared lines of
csrc/rows_gather_common.h in plain C++ -- against NumPy fancy indexing, the sampler, and every config refusal."""
import numpy as np
import pytest

from tumblr_emotions_amd import _lib, ops
from tumblr_emotions_amd.feature_cache import (FeatureSampler, check_feature_cache_config, check_feature_cache_fits, row_bytes,
                                               shard_rows)

from rows_gather_cases import CANARY, ROW_BYTES, make_tables

ON = {"feature_cache": "device", "feature_cache_gb": 1.0, "frozen_bn": True, "trainable_bn_beta": False}


def _unaligned(nbytes, rng, off):
    """A uint8 view of nbytes random bytes whose address is `off` past a multiple of 16."""
    raw = np.empty(nbytes + 32, np.uint8)
    start = (-raw.ctypes.data) % 16 + off
    v = raw[start:start + nbytes]
    v[:] = rng.integers(0, 256, nbytes, dtype=np.uint8)
    assert v.ctypes.data % 16 == off % 16
    return v


# ---- ds_rows_gather_host -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ntables", [1, 3, 8])
def test_host_gather_is_fancy_indexing(ntables):
    rng = np.random.default_rng(ntables)
    nrows, n = 13, 9
    rbs = (ROW_BYTES * 2)[:ntables]          # 4, 8, 20, 400, 163 072, 4, 8, 20
    index = rng.integers(0, nrows, n).astype(np.int64)
    index[3] = index[5] = index[0]           # repeated rows
    srcs, dsts = make_tables(rng, nrows, n, rbs)
    ops.rows_gather_host(list(zip(srcs, dsts)), index)
    for s, d in zip(srcs, dsts):
        assert np.array_equal(d, s[index])


def test_host_gather_takes_pointers_of_any_alignment():
    rng = np.random.default_rng(7)
    nrows, n = 6, 5
    index = np.array([5, 0, 0, 3, 2], np.int64)
    pairs = []
    for off, rb in ((1, 4), (2, 20), (3, 400), (5, 163072)):
        s = _unaligned(nrows * rb, rng, off).reshape(nrows, rb)
        d = _unaligned(n * rb, rng, off + 1).reshape(n, rb)
        pairs.append((s, d))
    raw = np.empty(8 * n + 16, np.uint8)                    # ... the index vector too
    ix = raw[3:3 + 8 * n]
    ix[:] = index.view(np.uint8)
    tables = (_lib.RowsTable * len(pairs))()
    for t, (s, d) in zip(tables, pairs):
        t.src, t.dst, t.row_bytes = s.ctypes.data, d.ctypes.data, s.shape[1]
    assert _lib.load().ds_rows_gather_host(tables, len(pairs), ix.ctypes.data, n, nrows) == 0
    for s, d in pairs:
        assert np.array_equal(d, s[index])


def test_an_index_out_of_range_leaves_its_row_untouched_in_every_table():
    rng = np.random.default_rng(11)
    nrows, n = 7, 6
    index = np.array([2, -1, 6, 7, 0, 1 << 40], np.int64)      # rows 1, 3, 5 name nothing
    srcs, dsts = make_tables(rng, nrows, n, (8, 400, 163072))
    ops.rows_gather_host(list(zip(srcs, dsts)), index)
    for s, d in zip(srcs, dsts):
        for i, r in enumerate(index):
            want = s[r] if 0 <= r < nrows else np.full(s.shape[1], CANARY, np.uint8)
            assert np.array_equal(d[i], want), (s.shape[1], i)


def test_argument_errors_are_codes_with_a_text():
    lib = _lib.load()
    a = np.zeros(64, np.uint8)
    ix = np.zeros(2, np.int64)

    def tables(*rows):
        t = (_lib.RowsTable * max(len(rows), 1))()
        for e, (s, d, rb) in zip(t, rows):
            e.src, e.dst, e.row_bytes = s, d, rb
        return t

    p = a.ctypes.data
    good = (p, p + 32, 8)
    for fn, extra in ((lib.ds_rows_gather_host, ()), (lib.ds_rows_gather, (None,))):
        name = b"ds_rows_gather_host" if not extra else b"ds_rows_gather"
        for args in ((None, 1, ix.ctypes.data, 2, 4),                                  # no tables
                     (tables(good), 0, ix.ctypes.data, 2, 4),                        # ntables outside 1..8
                     (tables(*([good] * 9)), 9, ix.ctypes.data, 2, 4),
                     (tables(good), 1, None, 2, 4),                                  # no index
                     (tables(good), 1, ix.ctypes.data, 0, 4),                        # n < 1
                     (tables(good), 1, ix.ctypes.data, 2, 0),                        # nrows < 1
                     (tables((None, p, 8)), 1, ix.ctypes.data, 2, 4),                # a null table
                     (tables((p, None, 8)), 1, ix.ctypes.data, 2, 4),
                     (tables(good, (p, p, 6)), 2, ix.ctypes.data, 2, 4),             # row_bytes not a multiple of 4
                     (tables((p, p, 0)), 1, ix.ctypes.data, 2, 4),
                     (tables((p, p, -4)), 1, ix.ctypes.data, 2, 4),
                     (tables((p, p, 1 << 34)), 1, ix.ctypes.data, 2, 4)):            # more than 2^31 units in one launch
            lib.ds_rows_gather_host(tables(good), 1, ix.ctypes.data, 1, 4)            # (a good call in between)
            assert fn(*args, *extra) == -1, args                                       # DS_ERR_ARG
            assert lib.ds_last_error().startswith(name + b":"), lib.ds_last_error()
    assert not a.any()                        # nothing was written
    # the device entry also refuses misaligned pointers, before any launch
    assert lib.ds_rows_gather(tables((p + 2, p + 32, 8)), 1, ix.ctypes.data, 2, 4, None) == -1
    assert b"4-byte aligned" in lib.ds_last_error()
    with pytest.raises(ValueError, match="multiple of 4"):
        ops.rows_gather_host([(np.zeros((4, 6), np.uint8), np.zeros((2, 6), np.uint8))], ix)
    with pytest.raises(ValueError, match="1 to 8"):
        ops.rows_gather_host([], ix)


# ---- the sampler -------------------------------------------------------------------------------------------------------------
def test_a_pass_is_a_permutation_of_the_shard_and_seeds_repeat():
    s = FeatureSampler(103, 8, seed=5)
    assert s.shard == 103 and s.steps_per_pass == 12
    for p in range(3):
        assert sorted(s.permutation(p)) == list(range(103))
    assert not np.array_equal(s.permutation(0), s.permutation(1))
    t = FeatureSampler(103, 8, seed=5)
    for step in (0, 11, 12, 30):
        assert np.array_equal(s.indices(step), t.indices(step)) and s.indices(step).dtype == np.int64
    assert not np.array_equal(FeatureSampler(103, 8, seed=6).permutation(0), s.permutation(0))
    # a pass's steps are disjoint slices of its permutation, the tail (103 - 96 = 7 rows) is dropped, then the next pass starts
    seen = np.concatenate([s.indices(k) for k in range(12)])
    assert np.array_equal(seen, s.permutation(0)[:96]) and len(set(seen)) == 96
    assert np.array_equal(s.indices(12), s.permutation(1)[:8]) and s.locate(12) == (1, 0) and s.locate(13) == (1, 8)


def test_two_ranks_are_disjoint_cover_everything_and_step_alike_for_odd_n():
    N = 11
    a, b = FeatureSampler(N, 2, rank=0, world=2, seed=1), FeatureSampler(N, 2, rank=1, world=2, seed=1)
    assert (a.shard, b.shard) == (6, 5) == (shard_rows(N, 0, 2), shard_rows(N, 1, 2))
    assert a.steps_per_pass == b.steps_per_pass == 2             # (11 // 2) // 2: the shorter shard's count on both
    ga = set(a.rank + a.permutation(0) * 2)
    gb = set(b.rank + b.permutation(0) * 2)
    assert not (ga & gb) and ga | gb == set(range(N))
    assert set(a.global_indices(0)) <= ga and set(b.global_indices(1)) <= gb
    assert not np.array_equal(a.permutation(0)[:5], b.permutation(0))      # the ranks draw their own permutations
    assert shard_rows(3, 5, 8) == 0


def test_clones_multiply_the_rows_of_a_step():
    one, four = FeatureSampler(100, 8), FeatureSampler(100, 8 * 4)
    assert one.steps_per_pass == 12 and four.steps_per_pass == 3 and four.indices(0).shape == (32,)
    assert np.array_equal(four.indices(1), four.permutation(0)[32:64])
    with pytest.raises(ValueError, match="no step"):
        FeatureSampler(10, 16)
    with pytest.raises(ValueError):
        FeatureSampler(10, 2, rank=2, world=2)


# ---- config ------------------------------------------------------------------------------------------------------------------
def test_the_config_check_answers_without_a_device():
    assert check_feature_cache_config({}) is None and check_feature_cache_config({"feature_cache": "none", "augment": True}) is None
    assert check_feature_cache_config(ON) == 10 ** 9
    assert check_feature_cache_config(dict(ON, feature_cache_gb=2)) == 2 * 10 ** 9
    bad = [{"feature_cache": "host"}, {"feature_cache_gb": None}, {"feature_cache_gb": 0}, {"feature_cache_gb": True},
           {"feature_cache_gb": "8"}, {"frozen_bn": False}, {"trainable_bn_beta": True}, {"augment": True}, {"synthetic": True},
           {"train_all": True}, {"dtype": "bf16"}, {"dtype": "fp8"}, {"input_cache": "device", "input_cache_gb": 1.0},
           {"trainable_bn_beta": 0}]
    for change in bad:
        with pytest.raises(ValueError):
            check_feature_cache_config(dict(ON, **change))
    for missing in ("feature_cache_gb", "frozen_bn", "trainable_bn_beta"):      # no default stands in for any of them
        with pytest.raises(ValueError, match=missing):
            check_feature_cache_config({k: v for k, v in ON.items() if k != missing})
    with pytest.raises(ValueError, match="image tower"):
        check_feature_cache_config(ON, with_images=False)
    with pytest.raises(ValueError, match="must be a bool"):
        check_feature_cache_config({"trainable_bn_beta": "no"})


def test_a_dataset_beyond_the_budget_is_refused_with_the_size_it_needs():
    assert row_bytes(50) == 163072 + 400 + 32
    assert check_feature_cache_fits(11, 50, 10 ** 9) == 11 * 163504
    with pytest.raises(ValueError, match=r"50000 records need 8\.175 GB .* allows 8\.000"):
        check_feature_cache_fits(50000, 50, int(8e9))


def test_the_front_ends_refuse_before_they_touch_a_device(tmp_path):
    from tumblr_emotions_amd.image_model.im_model import train_image_model
    from tumblr_emotions_amd.image_text_model.im_text_rnn_model import train_deep_sentiment
    for train in (train_image_model, train_deep_sentiment):
        for change in ({"augment": True}, {"frozen_bn": False}, {"feature_cache_gb": None}, {"synthetic": True}):
            with pytest.raises(ValueError, match="feature_cache"):
                train(None, str(tmp_path / "t"), 1, config=dict(ON, dataset_dir=str(tmp_path), **change))


# ---- the same host code, sanitised, in a program of its own --------------------------------------------------------------------
def test_sanitised_host_statement_survives_random_launches(tmp_path):
    import os
    import subprocess
    from test_input_cache_cpu import ROOT, _compiler
    exe = str(tmp_path / "rows_gather_host_driver")
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
                            os.path.join(ROOT, "tests", "rows_gather_host_driver.cpp"),
                            os.path.join(ROOT, "tumblr_emotions_amd", "csrc", "rows_gather_host.cpp"), "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0")
    run = subprocess.run([exe, "150", "20261020"], capture_output=True, text=True, env=env, timeout=300)
    assert run.returncode == 0, (run.returncode, run.stdout[-2000:], run.stderr[-6000:])
    assert "ERROR" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-6000:]
    launches, copied, skipped = [int(x) for x in run.stdout.split()[1::2]]
    assert launches == 150 and copied > 300 and skipped > 50
