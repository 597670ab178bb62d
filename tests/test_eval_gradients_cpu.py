"""Moving-statistics (is_training=False) gradients without a GPU: the three new entry points are exported, declared and bound;
they refuse bad arguments with an error code and a message before anything is launched; and the fp64 formula the GPU tests
compare the kernels against is what torch.autograd gives for batch_norm_infer + ReLU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from eval_grad_ref import bn_infer_relu_bwd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ds_bn_infer_bwd_apply", "ds_bn_pool_infer_bwd_apply", "ds_token_dot")
FAKE = C.c_void_p(0x10000)          # a non-null, 16-byte aligned address that no refused call dereferences


@pytest.fixture(scope="module")
def lib():
    from tumblr_emotions_amd import _lib
    if not (os.path.exists(_lib.LIB_PATH) and os.path.exists(_lib.TUNING_LIB_PATH)):
        subprocess.run(["make", "-C", os.path.join(ROOT, "tumblr_emotions_amd", "csrc"), "-j4"], check=True)
    return _lib


def test_new_entry_points_are_exported_declared_and_bound(lib):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ds_kernels.h")).read(), flags=re.S)
    dll = C.CDLL(lib.LIB_PATH)
    for n in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % n, header), "%s is not declared in ds_kernels.h" % n
        assert hasattr(dll, n), "libds_kernels.so lacks %s" % n
        assert n in lib.SIGNATURES
    from tumblr_emotions_amd import ops
    for n in ("bn_infer_bwd_apply", "bn_pool_infer_bwd_apply", "token_dot"):
        assert callable(getattr(ops, n))


def _segs(lib, nseg, C_):
    sg = lib.Segments()
    sg.nseg = nseg
    for i in range(min(nseg, 4)):
        sg.c_begin[i], sg.c_end[i], sg.ld[i], sg.ptr[i] = (0, C_, C_, FAKE.value) if i == 0 else (C_, C_, C_, FAKE.value)
    return sg


def _refused(l, rc, name):
    assert rc != 0
    assert name.encode() in l.ds_last_error()


def test_bn_infer_bwd_apply_refuses_bad_arguments(lib):
    l = lib.load()
    ok = _segs(lib, 1, 8)
    f = l.ds_bn_infer_bwd_apply
    _refused(l, f(None, 8, C.byref(ok), 4, 8, FAKE, FAKE, FAKE, None), "ds_bn_infer_bwd_apply")          # null z
    _refused(l, f(FAKE, 8, C.byref(ok), 4, 8, None, FAKE, FAKE, None), "ds_bn_infer_bwd_apply")          # null rstd
    _refused(l, f(FAKE, 8, C.byref(ok), 4, 8, FAKE, FAKE, None, None), "ds_bn_infer_bwd_apply")          # null dz
    _refused(l, f(FAKE, 8, None, 4, 8, FAKE, FAKE, FAKE, None), "ds_bn_infer_bwd_apply")                  # null segments
    _refused(l, f(FAKE, 6, C.byref(_segs(lib, 1, 6)), 4, 6, FAKE, FAKE, FAKE, None), "ds_bn_infer_bwd_apply")      # C % 4 != 0
    _refused(l, f(FAKE, 4, C.byref(ok), 4, 8, FAKE, FAKE, FAKE, None), "ds_bn_infer_bwd_apply")          # ldz < C
    _refused(l, f(FAKE, 8, C.byref(_segs(lib, 5, 8)), 4, 8, FAKE, FAKE, FAKE, None), "ds_bn_infer_bwd_apply")      # nseg > 4
    _refused(l, f(FAKE, 8, C.byref(_segs(lib, 1, 4)), 4, 8, FAKE, FAKE, FAKE, None), "ds_bn_infer_bwd_apply")      # 4 of 8 channels covered
    _refused(l, f(C.c_void_p(0x10004), 8, C.byref(ok), 4, 8, FAKE, FAKE, FAKE, None), "ds_bn_infer_bwd_apply")    # misaligned z


def test_bn_pool_infer_bwd_apply_refuses_bad_arguments(lib):
    l = lib.load()
    f = l.ds_bn_pool_infer_bwd_apply
    geo = (2, 9, 9, 8, 0, 0, 5, 5)
    _refused(l, f(None, FAKE, FAKE, *geo, FAKE, FAKE, FAKE, None), "ds_bn_pool_infer_bwd_apply")
    _refused(l, f(FAKE, None, FAKE, *geo, FAKE, FAKE, FAKE, None), "ds_bn_pool_infer_bwd_apply")
    _refused(l, f(FAKE, FAKE, None, *geo, FAKE, FAKE, FAKE, None), "ds_bn_pool_infer_bwd_apply")
    _refused(l, f(FAKE, FAKE, FAKE, *geo, FAKE, FAKE, None, None), "ds_bn_pool_infer_bwd_apply")
    _refused(l, f(FAKE, FAKE, FAKE, 2, 9, 9, 6, 0, 0, 5, 5, FAKE, FAKE, FAKE, None), "ds_bn_pool_infer_bwd_apply")     # C % 4 != 0
    _refused(l, f(FAKE, FAKE, FAKE, 2, 12, 9, 8, 0, 0, 5, 5, FAKE, FAKE, FAKE, None), "ds_bn_pool_infer_bwd_apply")    # H > 2 OH: not a stride-2 pool


def test_token_dot_refuses_bad_arguments(lib):
    l = lib.load()
    f = l.ds_token_dot
    _refused(l, f(None, FAKE, FAKE, FAKE, 2, 3, 4, None), "ds_token_dot")
    _refused(l, f(FAKE, None, FAKE, FAKE, 2, 3, 4, None), "ds_token_dot")
    _refused(l, f(FAKE, FAKE, None, FAKE, 2, 3, 4, None), "ds_token_dot")
    _refused(l, f(FAKE, FAKE, FAKE, None, 2, 3, 4, None), "ds_token_dot")
    _refused(l, f(FAKE, FAKE, FAKE, FAKE, 0, 3, 4, None), "ds_token_dot")
    _refused(l, f(FAKE, FAKE, FAKE, FAKE, 2, 3, 0, None), "ds_token_dot")


def test_the_fp64_formula_is_autograd_of_batch_norm_infer_and_relu():
    from oracle import tf_semantics as S
    from oracle.torch_ref import batch_norm_infer
    rng = np.random.RandomState(7)
    M, C_ = 3, 5
    z = rng.standard_normal((M, C_))
    dy = rng.standard_normal((M, C_))
    beta, mm, mv = rng.normal(0, 0.3, C_), rng.normal(0, 0.5, C_), rng.uniform(0.5, 2.0, C_)
    zt = torch.tensor(z.T.reshape(1, C_, M, 1), dtype=torch.float64, requires_grad=True)          # NCHW, as the oracle has it
    y = torch.relu(batch_norm_infer(zt, torch.tensor(beta), torch.tensor(mm), torch.tensor(mv)))
    (g,) = torch.autograd.grad((y * torch.tensor(dy.T.reshape(1, C_, M, 1))).sum(), zt)
    rstd = 1.0 / np.sqrt(mv + S.BN_EPS)
    shift = beta - mm * rstd
    got = bn_infer_relu_bwd(z, dy, rstd, shift)
    assert (got != 0).any() and (got == 0).any()          # both sides of the ReLU occur
    np.testing.assert_allclose(got, g.numpy().reshape(C_, M).T, rtol=1e-12, atol=0)
