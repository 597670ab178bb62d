"""The table shapes of ds_rows_gather, shared by test_feature_cache_cpu.py (the host statement against NumPy fancy
indexing) and test_feature_cache_gpu.py (the kernel against the host statement)."""
import numpy as np

# bytes per row: the int64 scalars' 8, the smallest row, one that is no multiple of 8 or 16, a text row, a feature row
ROW_BYTES = (4, 8, 20, 400, 163072)
CANARY = 0xA5


def make_tables(rng, nrows, n, row_bytes):
    """(sources, destinations): uint8 [nrows, rb] of random bytes and [n, rb] filled with CANARY, one pair per entry."""
    srcs = [rng.integers(0, 256, (nrows, rb), dtype=np.uint8) for rb in row_bytes]
    dsts = [np.full((n, rb), CANARY, np.uint8) for rb in row_bytes]
    return srcs, dsts


def host_reference(srcs, index, n):
    """What ds_rows_gather_host leaves in CANARY-filled destinations (computed once per case, read-only afterwards)."""
    from tumblr_emotions_amd import ops
    dsts = [np.full((n, s.shape[1]), CANARY, np.uint8) for s in srcs]
    ops.rows_gather_host(list(zip(srcs, dsts)), np.ascontiguousarray(index, np.int64), nrows=srcs[0].shape[0])
    for d in dsts:
        d.setflags(write=False)
    return dsts
