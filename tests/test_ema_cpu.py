"""Moving averages of the trained variables, the parts that need no device: the refused configurations, the
decay schedule and its fp32 rate, the shadow buffer of the parameter store, and the C ABI of the two new entry points."""
import ctypes
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import ema_ref as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ds_adam_tf_ema", "ds_adam_tf_clipped_ema")


def test_check_ema_config_accepts_a_float_between_zero_and_one_only():
    from tumblr_emotions_amd.net import check_ema_config
    from tumblr_emotions_amd.training import ema_net_kwargs
    assert check_ema_config() is None and check_ema_config(None) is None
    for ok in (0.9999, 0.5, 1e-9, np.float32(0.25), np.float64(0.999)):
        got = check_ema_config(ok)
        assert type(got) is float and got == float(ok)
        assert ema_net_kwargs({"moving_average_decay": ok}) == {"moving_average_decay": float(ok)}
    for bad in (0, 1, 0.0, 1.0, -0.5, 1.5, float("nan"), float("inf"), True, False, np.bool_(True), "0.9", [0.9], 2):
        with pytest.raises(ValueError, match="moving_average_decay"):
            check_ema_config(bad)
        with pytest.raises(ValueError, match="moving_average_decay"):
            ema_net_kwargs({"moving_average_decay": bad})
    assert ema_net_kwargs({}) == {} and ema_net_kwargs({"moving_average_decay": None}) == {}
    with pytest.raises(NotImplementedError, match="fp32"):
        ema_net_kwargs({"moving_average_decay": 0.9, "dtype": "bf16"})
    assert ema_net_kwargs({"moving_average_decay": 0.9, "dtype": "f32"}) == {"moving_average_decay": 0.9}


def test_the_model_constructor_refuses_before_it_asks_for_a_device():
    from tumblr_emotions_amd.net import SentimentNet
    for bad in (0.0, 1.0, True, "0.9", 3):
        with pytest.raises(ValueError, match="moving_average_decay"):
            SentimentNet(mode="text", moving_average_decay=bad)
    for dtype in ("bf16", "fp8"):
        with pytest.raises(NotImplementedError, match="moving_average_decay is implemented for the fp32 configuration"):
            SentimentNet(mode="joint", moving_average_decay=0.9999, dtype=dtype)


def test_schedule_of_decay_0_9999():
    """decay_1 = 2/11, decay_2 = 1/4, decay_10 = 0.55, and 0.9999 from t = 89990 on: (1 + t) / (10 + t) >= 0.9999 exactly when
    t >= 89990 (equality there, as rationals of the decimal 0.9999)."""
    from tumblr_emotions_amd.net import ema_decay
    d = 0.9999
    for t, want in ((1, Fraction(2, 11)), (2, Fraction(1, 4)), (10, Fraction(11, 20))):
        assert E.decay_exact(d, t) == want
        assert ema_decay(d, t) == np.float32(float(want)) and type(ema_decay(d, t)) is np.float32
    assert Fraction(1 + 89990, 10 + 89990) == Fraction(9999, 10000) and Fraction(89990, 89999) < Fraction(9999, 10000)
    # (one step earlier the schedule is still the smaller one -- in double; 1.2e-9 apart, the two round to one fp32 number)
    assert 89990.0 / 89999.0 < d and ema_decay(d, 89989) == np.float32(89990.0 / 89999.0)
    assert ema_decay(d, 80000) < np.float32(d)
    for t in (89990, 89991, 10 ** 6, 10 ** 9):
        assert ema_decay(d, t) == np.float32(d), t
    for t in list(range(1, 200)) + [89988, 89989, 89990, 89991]:
        assert ema_decay(d, t).tobytes() == E.decay32(d, t).tobytes()
    # decay 0.5: the min changes sides at t = 8 ((1 + 8) / (10 + 8) = 1/2)
    assert [float(ema_decay(0.5, t)) for t in (7, 8, 9)] == [float(np.float32(8.0 / 17.0)), 0.5, 0.5]


def test_rate_is_formed_in_fp32():
    """rate_t = 1.0f - (float)decay_t, not (float)(1 - decay_t): the two differ in the last bit for most t."""
    from tumblr_emotions_amd.net import ema_rate
    differ = 0
    for decay in (0.9999, 0.5, 0.999):
        for t in list(range(1, 300)) + [89989, 89990, 10 ** 6]:
            r = ema_rate(decay, t)
            assert type(r) is np.float32
            d32 = np.float32(min(decay, (1.0 + t) / (10.0 + t)))
            assert r.tobytes() == np.float32(np.float32(1.0) - d32).tobytes() == E.rate32(decay, t).tobytes()
            assert 0.0 < float(r) < 1.0
            differ += r != np.float32(1.0 - min(decay, (1.0 + t) / (10.0 + t)))
    assert differ > 0
    assert float(ema_rate(0.9999, 1)) == float(np.float32(1.0) - np.float32(2.0 / 11.0))


def test_reference_update_stays_inside_its_own_fp64_bound():
    """The bound the GPU test gates with holds for the NumPy fp32 restatement itself, and is tight: a restatement with the
    operations in another order (s * (1 - r) + w * r) leaves it."""
    rng = np.random.RandomState(0)
    n = 1 << 18
    s = (rng.choice([-1, 1], n) * 10.0 ** rng.uniform(-6, 1, n)).astype(np.float32)
    w = (rng.choice([-1, 1], n) * 10.0 ** rng.uniform(-6, 1, n)).astype(np.float32)
    for rate in (0.1, 0.01, 1e-4, 9.0 / 11.0):
        r = np.float32(rate)
        err = np.abs(E.update32(s, w, r).astype(np.float64) - E.update64(s, w, r))
        assert (err <= E.bound64(s, w, r)).all()
        other = (s * (np.float32(1) - r) + w * r).astype(np.float32)
        assert not (np.abs(other.astype(np.float64) - E.update64(s, w, r)) <= E.bound64(s, w, r)).all()
    assert np.array_equal(E.update32(s, w, 0.0), s)


def test_store_keeps_shadows_only_when_asked_and_round_trips_them():
    from tumblr_emotions_amd.params import ParamStore
    st = ParamStore(device="cpu")
    st.declare("a", (3,), True, l2=True)
    st.declare("frozen", (7,), False)
    st.declare("fused", (1, 1, 5, 12), True, columns=[("f0", 0, 5), ("f1", 5, 6), ("f2", 6, 12)])
    st.finalize()
    assert st.ema is None
    with pytest.raises(RuntimeError, match="moving"):
        st.state_dict(which="ema")
    st.reset_ema()                     # nothing to reset: still none
    assert st.ema is None
    rng = np.random.RandomState(1)
    st.theta.copy_(__import__("torch").from_numpy(rng.standard_normal(st.theta.numel()).astype(np.float32)))
    ema = st.enable_ema()
    assert ema is st.ema and ema.data_ptr() != st.theta.data_ptr() and ema.shape == st.theta.shape
    assert np.array_equal(ema.numpy(), st.theta.numpy())
    sd = {"a": rng.standard_normal(3), "f0": rng.standard_normal((1, 1, 5, 5)), "f1": rng.standard_normal((1, 1, 5, 1)),
          "f2": rng.standard_normal((1, 1, 5, 6))}
    theta = st.theta.clone()
    assert st.load_state_dict(sd, which="ema") == set(sd)
    assert np.array_equal(st.theta.numpy(), theta.numpy())              # the variables are not touched
    back = st.state_dict(which="ema")
    assert sorted(back) == sorted(sd)                                    # trainable names only, the fused tensor split
    for k in sd:
        assert np.array_equal(back[k], sd[k].astype(np.float32)), k
    fused = st.slot_view("fused", "ema")
    assert np.array_equal(fused[..., 5:6].numpy(), sd["f1"].astype(np.float32))
    assert sorted(st.state_dict()) == ["a", "f0", "f1", "f2", "frozen"]
    st.reset_ema()
    assert np.array_equal(st.ema.numpy(), st.theta.numpy())


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ds_kernels.h")).read(), flags=re.S)


def test_abi_of_the_two_entry_points():
    """Header, the library's dynamic symbols and the ctypes table agree, argument for argument."""
    from tumblr_emotions_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(ROOT, "tumblr_emotions_amd", "csrc"), "-j4"], check=True)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1].split("@")[0] for l in out.splitlines() if l.strip()}
    header = _header()
    ctype = {"float": ctypes.c_float, "int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32}
    for name in NEW:
        assert name in exported and name in _lib.SIGNATURES
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, header)
        assert m, "%s is not declared in ds_kernels.h" % name
        args = [a.strip() for a in m.group(1).split(",")]
        want = [ctypes.c_void_p if "*" in a else ctype[a.split()[0]] for a in args]
        res, argtypes = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and list(argtypes) == want, name
        # the arguments of the plain entry point plus shadow, ema_rate, ema_rate_dev
        m0 = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name[:-4], header)
        base = [" ".join(a.split()) for a in m0.group(1).split(",")]
        mine = [" ".join(a.split()) for a in args]
        assert [a for a in mine if a not in ("float *shadow", "float ema_rate", "const float *ema_rate_dev")] == base
        assert len(mine) == len(base) + 3
    # the existing entry points keep their signatures; the ABI version stays
    assert len(_lib.SIGNATURES["ds_adam_tf"][1]) == 14 and len(_lib.SIGNATURES["ds_adam_tf_clipped"][1]) == 20
    assert _lib.load().ds_version() == 4


def test_bad_arguments_are_refused_before_any_launch():
    """NULL shadow, a rate outside [0, 1] or NaN: DS_ERR_ARG on the host, with the function's name in ds_last_error() -- no
    device is needed to be refused."""
    from tumblr_emotions_amd import _lib
    lib = _lib.load()
    P = ctypes.c_void_p
    buf = (ctypes.c_float * 8)()
    p = ctypes.cast(buf, P)
    tab = ctypes.cast((ctypes.c_int64 * 8)(), P)
    for name in NEW:
        fn = getattr(lib, name)
        tail = (tab, 1, tab, 1, p, p, None) if "clipped" in name else (None,)

        def call(shadow, rate):
            return fn(p, p, p, p, shadow, 8, 4, 0.0, 1.0, 1e-3, None, rate, None, 0.9, 0.999, 1e-8, *tail)

        for shadow, rate in ((None, 0.5), (p, -1e-3), (p, 1.0 + 1e-6), (p, float("nan")), (p, float("inf"))):
            assert call(shadow, rate) == -1, (name, rate)      # DS_ERR_ARG
            assert name.encode() + b":" in lib.ds_last_error()
