"""Input gradients without a device: the stem's Conv2DBackpropInput plan (ds_conv_plan is host code), the NumPy
post-processing of class_visualisation (deprocess_image / blur_image, im_text_rnn_model.py:209-215) and the reference
caller's import line."""
import ctypes as C
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from tumblr_emotions_amd import _lib
    if not (os.path.exists(_lib.LIB_PATH) and os.path.exists(_lib.TUNING_LIB_PATH)):
        subprocess.run(["make", "-C", os.path.join(ROOT, "tumblr_emotions_amd", "csrc"), "-j4"], check=True)
    return _lib


def _plan(L, role, arith, opts, N, H, W, ci, co, k, s, ldx, ldz, flags=0):
    p = L.LayerPlanStruct()
    rc = L.load().ds_conv_plan(C.byref(p), role, arith, opts, N, H, W, ci, co, k, s, ldx, ldz, flags)
    return rc, p


@pytest.mark.parametrize("N,H,W,cin", [(256, 224, 224, 4), (3, 37, 29, 3), (1, 224, 224, 3)])
def test_stem_dgrad_plan_matches_the_forward_geometry(lib, N, H, W, cin):
    L = lib
    rc, fwd = _plan(L, L.DS_CONV_FWD, L.DS_ARITH_F32, L.DS_PLAN_PACKED_RGB, N, H, W, 4, 64, 7, 2, 4, 64, L.DS_EPI_STATS)
    assert rc == 0
    rc, p = _plan(L, L.DS_CONV_DGRAD, L.DS_ARITH_F32, L.DS_PLAN_PACKED_RGB, N, H, W, cin, 64, 7, 2, 64, 3)
    assert rc == 0, L.load().ds_last_error()
    assert p.family == L.DS_FAM_STEM_DGRAD == 9
    assert (p.d.OH, p.d.OW, p.d.pad_t, p.d.pad_l) == (fwd.d.OH, fwd.d.OW, fwd.d.pad_t, fwd.d.pad_l)
    assert p.alg_flops == fwd.alg_flops == 2.0 * N * fwd.d.OH * fwd.d.OW * 64 * 147
    assert p.partials == 0 and p.w_bytes == 0 and p.w_cin == cin and p.d.ldx == 64
    assert L.load().ds_conv_stem_dgrad_supported(H, W) == 1
    if H == 224:
        assert (p.d.OH, p.d.pad_t) == (112, 2)
    if H == 37:
        assert (p.d.OH, p.d.OW, p.d.pad_t, p.d.pad_l) == (19, 15, 3, 3)


def test_other_stride2_dgrads_stay_errors(lib):
    L = lib
    l = L.load()
    B = 8
    args = (B, 224, 224, 4, 64, 7, 2, 64, 3)
    # without DS_PLAN_PACKED_RGB the 7x7 / 2 dgrad is a plain stride-2 dgrad: not built
    assert _plan(L, L.DS_CONV_DGRAD, L.DS_ARITH_F32, 0, *args)[0] == -1
    # other arithmetic, epilogue flags, other output widths
    for arith in (L.DS_ARITH_BF16, L.DS_ARITH_FP8, L.DS_ARITH_F32X3):
        assert _plan(L, L.DS_CONV_DGRAD, arith, L.DS_PLAN_PACKED_RGB, *args)[0] == -1
        assert b"stem" in l.ds_last_error()
    for flags in (L.DS_EPI_STATS, L.DS_EPI_BNSUMS, L.DS_EPI_ACCUM):
        assert _plan(L, L.DS_CONV_DGRAD, L.DS_ARITH_F32, L.DS_PLAN_PACKED_RGB, *args, flags)[0] == -1
    assert _plan(L, L.DS_CONV_DGRAD, L.DS_ARITH_F32, L.DS_PLAN_PACKED_RGB, B, 224, 224, 4, 32, 7, 2, 64, 3)[0] == -1
    assert len(l.ds_last_error()) > 0
    # the plain 3x3 / 2 dgrad stays an error (as test_abi_cpu pins it)
    assert _plan(L, L.DS_CONV_DGRAD, L.DS_ARITH_F32, 0, B, 28, 28, 96, 128, 3, 2, 128, 96)[0] == -1
    # the family entry point checks its arguments without touching a device
    assert l.ds_conv_stem_dgrad(None, None, None, 1, 224, 224, 4, 64, None) == -1
    assert l.ds_conv_stem_dgrad_supported(0, 224) == 0


def test_deprocess_image_known_answer():
    from tumblr_emotions_amd.image_text_model.im_text_rnn_model import deprocess_image
    x = np.array([-1.0, 0.0, 0.5, 1.0, 2.5], np.float32)
    np.testing.assert_array_equal(deprocess_image(x), np.array([-0.75, -0.25, 0.0, 0.25, 1.0], np.float32))


def test_blur_image_is_gaussian_filter1d_on_axes_1_and_2():
    from tumblr_emotions_amd.image_text_model.im_text_rnn_model import blur_image
    rng = np.random.RandomState(4)
    x = rng.standard_normal((2, 17, 11, 3)).astype(np.float32)
    # known answer: a constant image stays constant (normalised kernel, edge-repeating reflection)
    np.testing.assert_allclose(blur_image(np.full((1, 9, 9, 3), 0.7, np.float32), 0.5), 0.7, rtol=1e-6)
    # sigma 0.5: radius 2, weights exp(-2 x^2) normalised; an impulse far from the edges shows them
    imp = np.zeros((1, 9, 9, 1), np.float64)
    imp[0, 4, 4, 0] = 1.0
    k = np.exp(-2.0 * np.arange(-2, 3) ** 2)
    k /= k.sum()
    np.testing.assert_allclose(blur_image(imp, 0.5)[0, 2:7, 2:7, 0], np.outer(k, k), rtol=1e-12)
    assert blur_image(x, 0.5).dtype == np.float32 and blur_image(x, 0.5).shape == x.shape
    try:
        from scipy.ndimage import gaussian_filter1d
    except ImportError:
        return      # (the comparison with scipy needs scipy; the package itself does not)
    for sigma in (0.5, 1, 2.5, 6):
        ref = gaussian_filter1d(gaussian_filter1d(x, sigma, axis=1), sigma, axis=2)
        np.testing.assert_allclose(blur_image(x, sigma), ref, rtol=1e-5, atol=1e-6)


def test_reference_caller_line_resolves_through_compat():
    compat = os.path.join(ROOT, "compat")
    code = ("from image_text_model.im_text_rnn_model import class_visualisation, blur_image, deprocess_image\n"
            "import tumblr_emotions_amd.image_text_model.im_text_rnn_model as M\n"
            "assert class_visualisation is M.class_visualisation and blur_image is M.blur_image\n"
            "assert deprocess_image is M.deprocess_image\n")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([compat, ROOT]))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_input_gradient_is_part_of_the_public_net():
    net = importlib.import_module("tumblr_emotions_amd.net")
    import inspect
    sig = inspect.signature(net.SentimentNet.input_gradient)
    assert list(sig.parameters)[:3] == ["self", "batch", "target"]
    for kw in ("is_training", "dropout_mask", "seed"):
        assert sig.parameters[kw].kind == inspect.Parameter.KEYWORD_ONLY
