"""Fused inference forward (DS_EPI_BN_RELU), the host side: new symbols, ctypes mirrors, the host-only plan decision for every
stride-1 Inception conv shape, argument errors before any launch, and the public switches.  No device needed."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

def inception_stride1_shapes():
    """(map, Cin, Cout, k) of every stride-1 conv launch behind the stem, walked from the engine's own stage table
    (engine_image.TOPOLOGY, the table the product builds its layers from): Conv2d_2b / 2c and, per Mixed block, the four 1x1
    convs as the reference declares them, the horizontally fused block-input 1x1 launch and the two 3x3 convs."""
    from tumblr_emotions_amd.engine_image import TOPOLOGY
    from tumblr_emotions_amd.ops import same_pad
    hw, c, shapes = 224, 3, []
    for item in TOPOLOGY:
        kind = item[0]
        if kind == "conv":
            k, stride, cout = item[2:5]
            if stride == 1:
                shapes.append((hw, c, cout, k))
            hw, c = same_pad(hw, k, stride)[0], cout
        elif kind == "maxpool":
            hw = same_pad(hw, item[2], item[3])[0]
        else:
            b0, (b1a, b1b), (b2a, b2b), b3 = item[2:6]
            shapes += [(hw, c, b0, 1), (hw, c, b1a, 1), (hw, c, b2a, 1), (hw, c, b3, 1), (hw, c, b0 + b1a + b2a, 1),
                       (hw, b1a, b1b, 3), (hw, b2a, b2b, 3)]
            c = b0 + b1b + b2b + b3
    return shapes


@pytest.fixture(scope="module")
def lib():
    from tumblr_emotions_amd import _lib
    _lib.load()
    return _lib


def _plan(L, role, N, H, W, ci, co, k, flags=0, ldx=None, ldz=None):
    p = L.LayerPlanStruct()
    rc = L.load().ds_conv_plan(C.byref(p), role, L.DS_ARITH_F32, 0, N, H, W, ci, co, k, 1, ci if ldx is None else ldx,
                               co if ldz is None else ldz, flags)
    assert rc == 0
    return p


def test_new_symbols_and_fields_exist(lib):
    dll = C.CDLL(lib.LIB_PATH)
    for n in ("ds_conv_plan_enable_bn_relu", "ds_bn_infer_prepare_multi"):
        assert hasattr(dll, n) and n in lib.SIGNATURES, n
    assert lib.DS_EPI_BN_RELU == 64
    names = [f[0] for f in lib.ConvIO._fields_]
    assert names[-2:] == ["scale", "shift"], names
    hdr = open(os.path.join(ROOT, "include", "ds_kernels.h")).read()
    io = re.search(r"typedef struct ds_conv_io \{(.*?)\} ds_conv_io;", hdr, flags=re.S).group(1)
    io = re.sub(r"/\*.*?\*/", "", io, flags=re.S)
    members = re.findall(r"\*?\s*(\w+);", io)
    assert members == names, (members, names)          # the ctypes mirror follows the header, field for field
    assert C.sizeof(lib.ConvIO) == 8 * len(names)
    assert [f[0] for f in lib.BnInferJob._fields_] == ["beta", "moving_mean", "moving_var", "C", "rstd", "shift"]


def test_the_shape_table_is_the_tower():
    shapes = inception_stride1_shapes()
    assert len(shapes) == 2 + 9 * 7
    assert shapes[0] == (56, 64, 64, 1) and shapes[1] == (56, 64, 192, 3)
    assert (28, 192, 64, 1) in shapes and (7, 832, 384 + 192 + 48, 1) in shapes and (7, 192, 384, 3) in shapes
    assert {hw for hw, _, _, _ in shapes} == {56, 28, 14, 7}


def test_toy_shapes_of_the_conv_checks_plan_or_stay_untouched(lib):
    """The stride-1 forward rows of the conv checks' table (odd extents, channel counts not divisible by 4): the epilogue is
    granted or the plan bytes are unchanged."""
    from test_conv_layers_cpu import SHAPES
    for role, N, H, W, ci, co, k, s in SHAPES:
        if role == "fwd" and s == 1:
            p = _plan(lib, lib.DS_CONV_FWD, N, H, W, ci, co, k)
            before = bytes(p)
            if lib.load().ds_conv_plan_enable_bn_relu(C.byref(p)) == 0:
                assert bytes(p) == before
            else:
                assert p.d.flags == lib.DS_EPI_BN_RELU


@pytest.mark.parametrize("N", [1, 32, 256])
def test_enable_bn_relu_for_every_stride1_inception_shape(lib, N):
    l = lib.load()
    for hw, ci, co, k in inception_stride1_shapes():
        p = _plan(lib, lib.DS_CONV_FWD, N, hw, hw, ci, co, k)
        fam = p.family
        assert l.ds_conv_plan_enable_bn_relu(C.byref(p)) == 1, (N, hw, ci, co, k, fam)
        assert p.d.flags == lib.DS_EPI_BN_RELU and p.partials == 0 and p.family == fam
        # Branch_3's pool on load accepts the epilogue as well
        if k == 1:
            q = _plan(lib, lib.DS_CONV_FWD, N, hw, hw, ci, co, k)
            if l.ds_conv_plan_enable_pool3(C.byref(q), C.c_void_p(4096)):
                q.d.flags, q.d.partials, q.partials = 0, 0, 0
                assert l.ds_conv_plan_enable_bn_relu(C.byref(q)) == 1, ("pool3", N, hw, ci, co)
                assert q.d.pool_argmax


def test_enable_bn_relu_refuses_and_leaves_the_plan_untouched(lib):
    l = lib.load()
    p = _plan(lib, lib.DS_CONV_DGRAD, 32, 28, 28, 192, 176, 1, ldx=176, ldz=192)
    before = bytes(p)
    assert l.ds_conv_plan_enable_bn_relu(C.byref(p)) == 0 and bytes(p) == before
    p = _plan(lib, lib.DS_CONV_DGRAD, 32, 28, 28, 96, 128, 3, ldx=128, ldz=96)
    before = bytes(p)
    assert l.ds_conv_plan_enable_bn_relu(C.byref(p)) == 0 and bytes(p) == before
    for k, ci, co in ((1, 192, 176), (3, 96, 128)):
        p = _plan(lib, lib.DS_CONV_FWD, 32, 28, 28, ci, co, k, flags=lib.DS_EPI_STATS)
        before = bytes(p)
        assert l.ds_conv_plan_enable_bn_relu(C.byref(p)) == 0 and bytes(p) == before
    assert l.ds_conv_plan_enable_bn_relu(None) == 0
    # the decision is made on the stride the launch will store with: F(4x4) needs 16-byte output pixels
    p = _plan(lib, lib.DS_CONV_FWD, 32, 28, 28, 96, 128, 3)
    assert p.family == lib.DS_FAM_WINO4
    p.d.ldz = 130
    before = bytes(p)
    assert l.ds_conv_plan_enable_bn_relu(C.byref(p)) == 0 and bytes(p) == before
    p.d.ldz = 256
    assert l.ds_conv_plan_enable_bn_relu(C.byref(p)) == 1
    # the flag is not a ds_conv_plan argument, and the 16-bit families do not carry it
    q = lib.LayerPlanStruct()
    assert l.ds_conv_plan(C.byref(q), 0, lib.DS_ARITH_F32, 0, 32, 28, 28, 96, 128, 3, 1, 96, 128, lib.DS_EPI_BN_RELU) == -1
    assert l.ds_conv_plan(C.byref(q), 0, lib.DS_ARITH_BF16, 0, 32, 28, 28, 96, 128, 3, 1, 96, 128, 0) == 0
    before = bytes(q)
    assert l.ds_conv_plan_enable_bn_relu(C.byref(q)) == 0 and bytes(q) == before


@pytest.mark.parametrize("shape", [(28, 192, 176, 1), (7, 832, 128, 1), (28, 96, 128, 3), (14, 24, 64, 3)])
def test_run_without_scale_is_an_error_before_any_launch(lib, shape):
    l = lib.load()
    hw, ci, co, k = shape
    p = _plan(lib, lib.DS_CONV_FWD, 32, hw, hw, ci, co, k)
    assert l.ds_conv_plan_enable_bn_relu(C.byref(p)) == 1
    io = lib.ConvIO()
    x = C.c_void_p(4096)
    assert l.ds_conv_run(C.byref(p), x, x, x, C.byref(io), None) != 0
    assert b"scale" in l.ds_last_error()
    io.scale = 4096                                   # shift still missing
    assert l.ds_conv_run(C.byref(p), x, x, x, C.byref(io), None) != 0 and b"shift" in l.ds_last_error()
    assert l.ds_conv_run(C.byref(p), x, x, x, None, None) != 0
    # the family-level entry points refuse the flag: it has no operands there
    assert l.ds_bn_infer_prepare_multi(None, 0, 1e-3, None) == -1 and b"ds_bn_infer_prepare_multi" in l.ds_last_error()


def test_predict_rejects_fused_training_and_non_f32():
    """The argument checks come before anything touches a device."""
    from tumblr_emotions_amd.net import SentimentNet
    import inspect
    sig = inspect.signature(SentimentNet.predict)
    assert list(sig.parameters)[1:] == ["batch", "is_training", "seed", "fused"] and sig.parameters["fused"].default is False

    class Stub:
        image = None
        dtype = "f32"
    s = Stub()
    with pytest.raises(ValueError, match="is_training"):
        SentimentNet.predict(s, {}, is_training=True, fused=True)
    s.dtype = "bf16"
    with pytest.raises(NotImplementedError, match="fp32"):
        SentimentNet.predict(s, {}, is_training=False, fused=True)


def test_run_evaluation_passes_the_config_key_to_predict(tmp_path, monkeypatch):
    """training.run_evaluation asks predict for the fused pass when config['fused_inference'] is set -- and never for
    mode 'train', which keeps batch statistics.  (A stub net: what is checked is the argument that reaches predict.)"""
    import torch
    from tumblr_emotions_amd import training
    seen = []

    class Net:
        def predict(self, batch, is_training=False, seed=None, fused=False):
            seen.append((is_training, fused))
            return torch.zeros(2, 3)

    class Model:
        net = Net()

        def next_batch(self, i):
            return {"labels": torch.zeros(2, dtype=torch.int64)}
    monkeypatch.setattr(training, "latest_checkpoint", lambda d: "x")
    monkeypatch.setattr(training, "load_checkpoint", lambda m, p: 0)
    for cfg, mode, want in (({"fused_inference": True}, "validation", (False, True)), ({"fused_inference": True}, "train", (True, False)),
                            ({}, "validation", (False, False))):
        m = Model()
        m.config = cfg
        del seen[:]
        training.run_evaluation(m, "ckpt", str(tmp_path), mode, 2, quiet=True)
        assert seen == [want, want], (cfg, mode, seen)
