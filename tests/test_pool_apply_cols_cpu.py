"""ds_bn_pool_bwd_apply_cols / ds_bn_bwd_apply_cols without a GPU: exported, declared and bound, and every bad argument is
refused with an error code and a message before anything is launched."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ds_bn_pool_bwd_apply_cols", "ds_bn_bwd_apply_cols")
FAKE = C.c_void_p(0x10000)          # a non-null, 16-byte aligned address that no refused call dereferences


@pytest.fixture(scope="module")
def lib():
    from tumblr_emotions_amd import _lib
    if not (os.path.exists(_lib.LIB_PATH) and os.path.exists(_lib.TUNING_LIB_PATH)):
        subprocess.run(["make", "-C", os.path.join(ROOT, "tumblr_emotions_amd", "csrc"), "-j4"], check=True)
    return _lib


def test_entry_points_are_exported_declared_and_bound(lib):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ds_kernels.h")).read(), flags=re.S)
    dll = C.CDLL(lib.LIB_PATH)
    from tumblr_emotions_amd import ops
    for n in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % n, header), "%s is not declared in ds_kernels.h" % n
        assert hasattr(dll, n), "libds_kernels.so lacks %s" % n
        assert n in lib.SIGNATURES
        assert callable(getattr(ops, n[3:]))
        assert "`%s`" % n in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def _refused(l, rc, name, word=None):
    assert rc != 0
    msg = l.ds_last_error()
    assert name.encode() in msg and (word is None or word.encode() in msg), msg


def _pool_args(**kw):
    """A call nothing is wrong with (2 x 9 x 9, the columns [8, 20) of a 20-wide 3x3/2 pool), then one argument replaced."""
    a = dict(z=FAKE, ldz=12, dz=FAKE, lddz=12, dpool=FAKE, argmax=FAKE, Cp=20, c0=8, N=2, H=9, W=9, pad_t=1, pad_l=1, OH=5, OW=5,
             ncols=12, mean=FAKE, rstd=FAKE, shift=FAKE, coef_g=FAKE, coef_gx=FAKE, k=3, stream=None)
    a.update(kw)
    return list(a.values())


def test_bn_pool_bwd_apply_cols_refuses_bad_arguments(lib):
    l = lib.load()
    f, name = l.ds_bn_pool_bwd_apply_cols, "ds_bn_pool_bwd_apply_cols"
    for p in ("z", "dz", "dpool", "argmax", "mean", "rstd", "shift", "coef_g", "coef_gx"):
        _refused(l, f(*_pool_args(**{p: None})), name, "null")
    _refused(l, f(*_pool_args(ncols=10)), name, "multiples of 4")                 # ncols % 4
    _refused(l, f(*_pool_args(c0=6)), name, "multiples of 4")                     # first column not 4-aligned
    _refused(l, f(*_pool_args(ldz=8)), name, "stride smaller")                    # z's stride smaller than the range
    _refused(l, f(*_pool_args(lddz=8)), name, "stride smaller")                   # dz's
    _refused(l, f(*_pool_args(Cp=16)), name, "stride smaller")                    # the pool's: 8 + 12 > 16
    _refused(l, f(*_pool_args(k=1)), name, "kernel size")
    _refused(l, f(*_pool_args(k=5)), name, "kernel size")
    _refused(l, f(*_pool_args(H=12)), name, "H > 2 OH")                           # not a stride-2 SAME pool
    _refused(l, f(*_pool_args(W=11)), name, "W > 2 OW")
    _refused(l, f(*_pool_args(k=2, H=10, OH=5, pad_t=1)), name, "H > 2 OH")       # 2x2/2 windows would leave row 9 out
    _refused(l, f(*_pool_args(z=C.c_void_p(0x10004))), name, "aligned")


def _full_pool_args(tail, **kw):
    """A ds_bn_pool_bwd_reduce / _apply call nothing is wrong with (2 x 9 x 9 x 8 behind a 3x3/2 pool), one argument replaced."""
    a = dict(z=FAKE, dpool=FAKE, argmax=FAKE, N=2, H=9, W=9, C=8, pad_t=1, pad_l=1, OH=5, OW=5, mean=FAKE, rstd=FAKE, shift=FAKE)
    a.update(kw)
    return list(a.values()) + [FAKE] * tail + [None]


@pytest.mark.parametrize("name,tail", [("ds_bn_pool_bwd_reduce", 1), ("ds_bn_pool_bwd_apply", 2)])
def test_bn_pool_bwd_reduce_and_apply_refuse_what_their_siblings_refuse(lib, name, tail):
    l = lib.load()
    call = getattr(l, name)

    def f(*a):
        rc = call(*a)
        assert rc == -1, "%s returned %d, not DS_ERR_ARG" % (name, rc)
        return rc

    _refused(l, f(*_full_pool_args(tail, z=C.c_void_p(0x10004))), name, "aligned")          # a pointer off by 4 bytes
    _refused(l, f(*_full_pool_args(tail, dpool=C.c_void_p(0x10004))), name, "aligned")
    _refused(l, f(*_full_pool_args(tail, rstd=C.c_void_p(0x10004))), name, "aligned")
    _refused(l, f(*_full_pool_args(tail, N=0)), name, "geometry")
    _refused(l, f(*_full_pool_args(tail, pad_t=2)), name, "geometry")
    _refused(l, f(*_full_pool_args(tail, H=12)), name, "H > 2 OH")                          # (refused before, too)
    _refused(l, f(*_full_pool_args(tail, C=6)), name)
    _refused(l, f(*_full_pool_args(tail, z=None)), name, "null")


def test_bn_bwd_apply_cols_refuses_bad_arguments(lib):
    l = lib.load()
    f, name = l.ds_bn_bwd_apply_cols, "ds_bn_bwd_apply_cols"
    sg = lib.Segments()
    sg.nseg = 1
    sg.c_begin[0], sg.c_end[0], sg.ld[0], sg.ptr[0] = 0, 8, 8, FAKE.value
    ok = [FAKE, 24, C.byref(sg), 4, 8, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, None]
    for i in (0, 5, 6, 7, 8, 9, 10):
        _refused(l, f(*[None if j == i else a for j, a in enumerate(ok)]), name)
    _refused(l, f(*[None if j == 2 else a for j, a in enumerate(ok)]), name)          # null segments
    _refused(l, f(*[4 if j == 1 else a for j, a in enumerate(ok)]), name)             # ldz < ncols
    _refused(l, f(*[6 if j == 4 else a for j, a in enumerate(ok)]), name)             # ncols % 4
    _refused(l, f(*[12 if j == 4 else a for j, a in enumerate(ok)]), name)            # 8 of 12 columns covered
    _refused(l, f(*[C.c_void_p(0x10004) if j == 9 else a for j, a in enumerate(ok)]), name)      # misaligned coef_gx
