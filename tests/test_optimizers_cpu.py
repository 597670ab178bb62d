"""slim's optimiser choice and learning-rate schedules, the parts that need no device: the refused
configurations, the C ABI of ds_opt_step and what it refuses before any launch, learning_rate_at against its fp32
restatement and an exact closed form, and the fp32 restatements of the four updates inside their own fp64 bound."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import optim_ref as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE = {"initial_lr": 1e-3, "decay_factor": 0.3, "batch_size": 32}


# ---- refused configurations ---------------------------------------------------------------------------------------------
def test_check_optimizer_config_defaults_and_epsilon():
    from tumblr_emotions_amd.net import check_optimizer_config
    assert check_optimizer_config() == {"optimizer": "adam", "opt_epsilon": 1e-8, "adam_beta1": 0.9, "adam_beta2": 0.999}
    assert check_optimizer_config("sgd") == {"optimizer": "sgd"}
    assert check_optimizer_config("momentum") == {"optimizer": "momentum", "momentum": 0.9}
    assert check_optimizer_config("rmsprop") == {"optimizer": "rmsprop", "opt_epsilon": 1.0, "momentum": 0.9,
                                                 "rmsprop_decay": 0.9}
    got = check_optimizer_config("rmsprop", opt_epsilon=1e-10, momentum=0, rmsprop_decay=np.float32(0.5))
    assert got == {"optimizer": "rmsprop", "opt_epsilon": 1e-10, "momentum": 0.0, "rmsprop_decay": 0.5}
    assert all(type(v) is float for k, v in got.items() if k != "optimizer")
    assert check_optimizer_config("adam", adam_beta1=0.0, adam_beta2=0.5, opt_epsilon=0.1)["adam_beta1"] == 0.0


def test_every_refused_optimizer_configuration_names_its_key():
    from tumblr_emotions_amd.net import check_optimizer_config
    from tumblr_emotions_amd.training import optimizer_net_kwargs
    for name in ("adamw", "RMSProp", "", None, 3):
        with pytest.raises(ValueError, match="optimizer.*'adam', 'sgd', 'momentum', 'rmsprop'"):
            check_optimizer_config(name)
        with pytest.raises(ValueError, match="optimizer"):
            optimizer_net_kwargs({"optimizer": name})
    for name in ("adadelta", "adagrad", "ftrl"):
        with pytest.raises(NotImplementedError, match=name):
            check_optimizer_config(name)
        with pytest.raises(NotImplementedError, match=name):
            optimizer_net_kwargs({"optimizer": name})
    nonsense = (float("nan"), float("inf"), -float("inf"), True, "0.9", [0.9], None)
    out_of_range = {"momentum": (-0.1, 1.0, 1.5), "rmsprop_decay": (0.0, 1.0, -0.5, 2), "adam_beta1": (-1e-3, 1.0),
                    "adam_beta2": (-1e-3, 1.0, 7), "opt_epsilon": (0.0, -1e-8)}
    reader = {"momentum": "momentum", "rmsprop_decay": "rmsprop", "adam_beta1": "adam", "adam_beta2": "adam",
              "opt_epsilon": "rmsprop"}
    for key, bads in out_of_range.items():
        for bad in bads + tuple(x for x in nonsense if not (x is None and key == "opt_epsilon")):
            with pytest.raises(ValueError, match=key):
                check_optimizer_config(reader[key], **{key: bad})
            with pytest.raises(ValueError, match=key):
                optimizer_net_kwargs({"optimizer": reader[key], key: bad})
    # a hyper-parameter for an optimiser that does not read it: silently ignored, a sweep over it would measure nothing
    unread = {"sgd": ("momentum", "rmsprop_decay", "adam_beta1", "adam_beta2", "opt_epsilon"),
              "momentum": ("rmsprop_decay", "adam_beta1", "adam_beta2", "opt_epsilon"),
              "rmsprop": ("adam_beta1", "adam_beta2"), "adam": ("momentum", "rmsprop_decay")}
    for name, keys in unread.items():
        for key in keys:
            with pytest.raises(ValueError, match=key):
                check_optimizer_config(name, **{key: 0.5})
            with pytest.raises(ValueError, match=key):
                optimizer_net_kwargs({"optimizer": name, key: 0.5})
            default = {"momentum": 0.9, "rmsprop_decay": 0.9, "adam_beta1": 0.9, "adam_beta2": 0.999, "opt_epsilon": 1e-8}[key]
            with pytest.raises(ValueError, match=key):      # in a config the key's presence is what counts
                optimizer_net_kwargs({"optimizer": name, key: default})
    with pytest.raises(ValueError, match="momentum"):
        optimizer_net_kwargs({"momentum": 0.5})                      # (no 'optimizer': adam)
    assert optimizer_net_kwargs({}) == {} and optimizer_net_kwargs(BASE) == {}
    assert optimizer_net_kwargs({"optimizer": "rmsprop", "opt_epsilon": 1.0, "momentum": 0.5}) == \
        {"optimizer": "rmsprop", "opt_epsilon": 1.0, "momentum": 0.5}


def test_the_model_constructor_refuses_before_it_asks_for_a_device():
    from tumblr_emotions_amd.net import SentimentNet
    with pytest.raises(ValueError, match="optimizer"):
        SentimentNet(mode="text", optimizer="lamb")
    with pytest.raises(NotImplementedError, match="ftrl"):
        SentimentNet(mode="text", optimizer="ftrl")
    with pytest.raises(ValueError, match="rmsprop_decay"):
        SentimentNet(mode="text", optimizer="rmsprop", rmsprop_decay=1.0)
    with pytest.raises(ValueError, match="adam_beta2"):
        SentimentNet(mode="text", optimizer="momentum", adam_beta2=0.99)
    with pytest.raises(ValueError, match="opt_epsilon"):
        SentimentNet(mode="joint", optimizer="adam", opt_epsilon=0.0, dtype="bf16")


def test_every_refused_schedule_configuration_names_its_key():
    from tumblr_emotions_amd.training import check_schedule_config, learning_rate_at
    assert check_schedule_config(BASE) is None and check_schedule_config(BASE, 1000) is None
    for key in ("learning_rate_decay_factor", "num_epochs_per_decay", "end_learning_rate"):
        with pytest.raises(ValueError, match=key + ".*learning_rate_decay_type"):
            check_schedule_config(dict(BASE, **{key: 0.5}))
        with pytest.raises(ValueError, match=key):
            learning_rate_at(dict(BASE, **{key: 0.5}), 1000, 0)
    for kind in ("cosine", "Fixed", 1, ""):
        with pytest.raises(ValueError, match="learning_rate_decay_type"):
            check_schedule_config(dict(BASE, learning_rate_decay_type=kind))
    for kind, key in (("fixed", "learning_rate_decay_factor"), ("fixed", "num_epochs_per_decay"), ("fixed", "end_learning_rate"),
                      ("exponential", "end_learning_rate"), ("polynomial", "learning_rate_decay_factor")):
        with pytest.raises(ValueError, match=key):
            check_schedule_config(dict(BASE, learning_rate_decay_type=kind, **{key: 0.5}))
    for key, kind, bads in (("learning_rate_decay_factor", "exponential", (0, -0.5, float("nan"), True, "0.9")),
                            ("num_epochs_per_decay", "polynomial", (0, -1, float("inf"), False, None)),
                            ("end_learning_rate", "polynomial", (-1e-9, float("nan"), "0", True))):
        for bad in bads:
            with pytest.raises(ValueError, match=key):
                check_schedule_config(dict(BASE, learning_rate_decay_type=kind, **{key: bad}))
    # decay_steps = int(31 / 32 * 1.0) = 0
    for kind in ("exponential", "polynomial"):
        with pytest.raises(ValueError, match="decay_steps"):
            check_schedule_config(dict(BASE, learning_rate_decay_type=kind, num_epochs_per_decay=1.0), 31)
        with pytest.raises(ValueError, match="decay_steps"):
            learning_rate_at(dict(BASE, learning_rate_decay_type=kind, num_epochs_per_decay=1.0), 31, 0)
    assert check_schedule_config(dict(BASE, learning_rate_decay_type="fixed"), 31) == ("fixed", None)
    assert check_schedule_config(dict(BASE, learning_rate_decay_type="exponential"), 96) == ("exponential", 6)


# ---- learning_rate_at ---------------------------------------------------------------------------------------------------
def _ts(ds):
    return (0, ds - 1, ds, ds + 1, 10 * ds)


def test_absent_key_is_the_per_epoch_rule():
    from tumblr_emotions_amd.training import learning_rate_at
    for num_samples, clones, world in ((96, 1, 1), (1000, 2, 1), (1000, 1, 2), (10, 1, 1)):
        cfg = dict(BASE, num_clones=clones) if clones > 1 else dict(BASE)
        nb = max(1, num_samples // (32 * clones * world))
        # the loop of run_training, as it has always been
        epoch, lr = 0, cfg["initial_lr"]
        for step in range(3 * nb + 2):
            if step % nb == 0:
                lr = cfg["initial_lr"] * cfg["decay_factor"] ** epoch
                epoch += 1
            got = learning_rate_at(cfg, num_samples, step, world=world)
            assert type(got) is float and got == lr, (num_samples, step)


SCHEDULES = [
    # the defaults of slim's flags with an initial_lr that is no fp32 number
    ("fixed", dict(BASE, learning_rate_decay_type="fixed"), 96),
    ("exp_defaults", dict(BASE, initial_lr=0.01, learning_rate_decay_type="exponential"), 96),
    ("exp_large", dict(BASE, initial_lr=0.045, learning_rate_decay_type="exponential", learning_rate_decay_factor=0.5,
                       num_epochs_per_decay=2.5), 1281167),
    # polynomial: initial - end and t / decay_steps are exact in fp32 (2^-7 - 2^-13; decay_steps = 8)
    ("poly_exact", dict(BASE, initial_lr=2.0 ** -7, learning_rate_decay_type="polynomial", end_learning_rate=2.0 ** -13), 128),
]


@pytest.mark.parametrize("name,cfg,num_samples", SCHEDULES, ids=[s[0] for s in SCHEDULES])
def test_learning_rate_at_is_the_fp32_restatement_and_within_2_ulps_of_exact(name, cfg, num_samples):
    """Why 2 ulps hold (spacing(x) > u |x|, u = 2^-24).  fixed: one cast.  exponential: the correctly rounded power and the
    product, relative error < 2u.  poly_exact: the difference initial - end, p = t / 8 and 1 - p are exact, which leaves the
    product ((initial - end)(1 - p) <= the result) and the sum: < 2u |result|."""
    from tumblr_emotions_amd.training import learning_rate_at
    ds = 1 if name == "fixed" else O.decay_steps(cfg, num_samples)
    assert ds == {"fixed": 1, "exp_defaults": 6, "exp_large": 100091, "poly_exact": 8}[name]
    seen = []
    for t in _ts(ds) + (1, 2, 3 * ds + 1):
        got = learning_rate_at(cfg, num_samples, t)
        assert type(got) is np.float32 and got == O.schedule32(cfg, num_samples, t), t
        ulps = O.ulps32(got, O.schedule_exact(cfg, num_samples, t))
        assert ulps <= 2.0, (t, ulps)
        seen.append(float(got))
    if name == "fixed":
        assert set(seen) == {float(np.float32(1e-3))}
    elif name.startswith("exp"):      # a staircase: flat until decay_steps, one factor down at it
        assert seen[0] == seen[1] == float(np.float32(cfg["initial_lr"])) and seen[2] == seen[3] < seen[0] and seen[4] < seen[3]
    else:
        assert seen[0] == 2.0 ** -7 and seen[1] > seen[2] == seen[3] == seen[4] == 2.0 ** -13


def test_polynomial_with_inexact_operands_stays_inside_its_derived_bound():
    """initial_lr = 1e-3, end = 1e-4, decay_steps = 6: D = initial - end, p = t / 6 and 1 - p are rounded.  With R the exact
    result: |error| <= 1.001 u (3 D (1 - p) + D p + R) -- the roundings of D, of 1 - p and of the product reach R through
    D (1 - p), that of p through D p, and the sum's is u R."""
    from tumblr_emotions_amd.training import learning_rate_at
    cfg = dict(BASE, learning_rate_decay_type="polynomial")
    worst = 0.0
    for t in _ts(6) + (1, 2, 3, 4):
        got = learning_rate_at(cfg, 96, t)
        assert got == O.schedule32(cfg, 96, t)
        exact = O.schedule_exact(cfg, 96, t)
        D = float(np.float32(1e-3)) - float(np.float32(1e-4))
        p = min(t, 6) / 6.0
        bound = 1.001 * O.U * (3 * D * (1 - p) + D * p + float(exact))
        err = abs(float(got) - float(exact))
        worst = max(worst, err / bound)
        assert err <= bound, (t, err / bound)
    print("polynomial, inexact operands: largest |error| / bound = %.4f" % worst)
    assert learning_rate_at(cfg, 96, 6) == learning_rate_at(cfg, 96, 60) == np.float32(1e-4)


# ---- the C ABI ----------------------------------------------------------------------------------------------------------
def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ds_kernels.h")).read(), flags=re.S)


def test_abi_of_ds_opt_step():
    """Header, the library's dynamic symbols and the ctypes table agree; the descriptor's fields too."""
    from tumblr_emotions_amd import _lib, ops
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(ROOT, "tumblr_emotions_amd", "csrc"), "-j4"], check=True)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1].split("@")[0] for l in out.splitlines() if l.strip()}
    assert "ds_opt_step" in exported and "ds_opt_step" in _lib.SIGNATURES
    header = _header()
    m = re.search(r"\bint\s+ds_opt_step\s*\(([^)]*)\)\s*;", header)
    assert m, "ds_opt_step is not declared in ds_kernels.h"
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert args[0] == "const ds_opt_desc *d"
    ctype = {"float": ctypes.c_float, "int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32}
    res, argtypes = _lib.SIGNATURES["ds_opt_step"]
    assert res is ctypes.c_int and argtypes[0] is ctypes.POINTER(_lib.OptDesc)
    assert list(argtypes[1:]) == [ctypes.c_void_p if "*" in a else ctype[a.split()[0]] for a in args[1:]]
    # the descriptor: every field of the header's struct, in its order, with its type
    body = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*ds_opt_desc\s*;", header).group(1)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        base = decl.replace("const", "").split()[0]
        for name in decl[decl.index(base) + len(base):].split(","):
            name = name.strip()
            fields.append((name.lstrip("*"), ctypes.c_void_p if name.startswith("*") else ctype[base]))
    assert fields == [(n, t) for n, t in _lib.OptDesc._fields_]
    kinds = dict(re.findall(r"(DS_OPT_[A-Z]+)\s*=\s*(\d)", header))
    assert kinds == {"DS_OPT_ADAM": "0", "DS_OPT_SGD": "1", "DS_OPT_MOMENTUM": "2", "DS_OPT_RMSPROP": "3"}
    assert ops.OPT_KINDS == {"adam": 0, "sgd": 1, "momentum": 2, "rmsprop": 3}
    # the four Adam entry points keep their signatures; the ABI version stays
    assert len(_lib.SIGNATURES["ds_adam_tf"][1]) == 14 and len(_lib.SIGNATURES["ds_adam_tf_clipped_ema"][1]) == 23
    assert _lib.load().ds_version() == 4


def test_bad_arguments_are_codes_not_exceptions():
    """A null descriptor, theta or g, n <= 0, n_wd outside [0, n], an unknown kind, a slot the kind reads being NULL, a
    clipped descriptor that lacks one of its parts, a rate outside [0, 1] beside a shadow: DS_ERR_ARG on the host, with the
    function's name in ds_last_error() -- no device is needed to be refused."""
    from tumblr_emotions_amd import _lib
    lib = _lib.load()
    P = ctypes.c_void_p
    p = ctypes.cast((ctypes.c_float * 8)(), P)
    tab = ctypes.cast((ctypes.c_int64 * 8)(), P)

    def desc(kind=3, **kw):
        d = _lib.OptDesc()
        d.kind, d.lr, d.b1, d.b2, d.eps, d.momentum, d.rho = kind, 1e-3, 0.9, 0.999, 1.0, 0.9, 0.9
        for k, v in kw.items():
            setattr(d, k, v)
        return ctypes.byref(d)

    def refused(d, theta=p, g=p, s0=p, s1=p, n=8, n_wd=4):
        rc = lib.ds_opt_step(d, theta, g, s0, s1, n, n_wd, 0.0, 1.0, None)
        return rc == -1 and b"ds_opt_step:" in lib.ds_last_error()

    clip = dict(segments=tab, chunks=tab, nseg=1, nchunks=1, factors=p, flags=p)
    assert refused(None)
    assert refused(desc(), theta=None) and refused(desc(), g=None)
    assert refused(desc(), n=0) and refused(desc(), n=-8) and refused(desc(), n_wd=9) and refused(desc(), n_wd=-1)
    for kind in (-1, 4, 100):
        assert refused(desc(kind))
    assert refused(desc(0), s0=None) and refused(desc(0), s1=None)             # adam reads both
    assert refused(desc(2), s0=None)                                           # momentum its accumulator
    assert refused(desc(3), s0=None) and refused(desc(3), s1=None)             # rmsprop both
    for missing in clip:
        part = {k: v for k, v in clip.items() if k != missing}
        for kind in range(4):
            assert refused(desc(kind, **part)), (missing, kind)
    for rate in (-1e-3, 1.0 + 1e-6, float("nan"), float("inf")):
        assert refused(desc(1, shadow=p, ema_rate=rate))


# ---- the restatements inside their own bounds ---------------------------------------------------------------------------
def test_fp32_restatements_stay_inside_their_own_fp64_bounds():
    """The bounds the GPU test gates rmsprop's mom and theta with hold for the NumPy fp32 restatement itself, on the inputs
    of that test, for every kind and both epsilons; the worst ratios are printed."""
    from test_ema_gpu import Flat
    worst = {}

    def gate(kind, what, got, q):
        r = O.worst_ratio(got, q)
        worst[(kind, what)] = max(worst.get((kind, what), 0.0), r)
        assert r <= 1.0, (kind, what, r)

    for n in (4, 1020, 1028, 2048 * 256 + 260):
        c = Flat(n, seed=n % 1000)
        for factor in (None, np.float32(0.37)):
            gi = O.g_eff32(c.theta, c.g, c.n_wd, 0.25, 0.5, factor)
            for lr in (3e-3, 0.5):
                gate("sgd", "theta", O.sgd32(c.theta, gi, lr), O.sgd64(c.theta, gi, lr))
                w, a = O.momentum32(c.theta, c.m, gi, lr, 0.9)
                qw, qa = O.momentum64(c.theta, c.m, gi, lr, 0.9)
                gate("momentum", "theta", w, qw), gate("momentum", "acc", a, qa)
                for eps in (1.0, 1e-10):
                    w, mom, ms = O.rmsprop32(c.theta, c.m, c.v, gi, lr, 0.9, 0.9, eps)
                    qw, qmom, qms = O.rmsprop64(c.theta, c.m, c.v, gi, lr, 0.9, 0.9, eps)
                    gate("rmsprop", "theta", w, qw), gate("rmsprop", "mom", mom, qmom), gate("rmsprop", "ms", ms, qms)
                    assert (ms > 0).all()
                w, m, v = O.adam32(c.theta, c.m, c.v, gi, lr, 0.9, 0.999, 1e-8)
                qw, qm, qv = O.adam64(c.theta, c.m, c.v, gi, lr, 0.9, 0.999, 1e-8)
                gate("adam", "theta", w, qw), gate("adam", "m", m, qm), gate("adam", "v", v, qv)
    for k in sorted(worst):
        print("%-8s %-5s largest |fp32 - fp64| / bound = %.4f" % (k + (worst[k],)))
    # usable: not vacuous -- a restatement with rmsprop's operations in another order (ms rho + g^2 (1 - rho)) leaves it
    c = Flat(1 << 16, seed=7)
    gi = O.g_eff32(c.theta, c.g, c.n_wd, 0.25, 0.5)
    _, _, qms = O.rmsprop64(c.theta, c.m, c.v, gi, 3e-3, 0.9, 0.9, 1.0)
    f = np.float32
    other = (c.v * f(0.9) + (gi * gi) * (f(1) - f(0.9))).astype(np.float32)
    assert O.worst_ratio(other, qms) > 1.0
