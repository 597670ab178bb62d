"""Every conv plan the image engine builds, replayed layer by layer against an fp64 reference of the same operation.

The kernel tests call the families' own entry points at N <= 5 on small maps; the model tests run the product path end to
end behind loose 16-bit gates.  Here the plans come from SentimentNet(mode="image") itself after one step -- family,
geometry, split-K slices and workspace, ldx / ldz concat strides, x_dtype / z_dtype storage, the STATS / BNSUMS / ACCUM
epilogues as the engine left them -- so what runs is exactly the launch the product makes, on buffers the test owns.  The
on-load fusions (norm-on-load, bnb, pool3, mask_rstd / mask_shift) point at engine buffers and have their
own bit-identity tests: they are cleared, and the partial count is re-planned for the plain launch.

Configurations (each reaches launches the others do not):
  f32   B = 256 (headline), 32 (per-rank share: split-K F(4x4) slices), 128 (only the layers whose family or split-K
        count differs from both), B = 1 through input_gradient (unpooled stem, the stem's input gradient, split-K at N = 1)
  f32 with mul3 (f32x3)            B = 32: the forward 1x1 convs on three bf16 pieces
  f32 with winograd4 off            B = 32: F(2x2) Winograd (DS_PLAN_NO_WINO4)
  bf16, fp8                         B = 256 and 32: register-direct bf16 / fp8, F(4x4) on bf16 pieces, 16-bit x / dz / z storage
Mixed_5c's weight gradients (the trainable layers) are checked at each f32 batch against S.conv2d_same_bwd_filter.

Gates: those of the family's kernel test (tests/test_kernels_gpu.py), per element as a fraction of max|ref| over the sampled
images, and 2e-3 (1e-3 where the kernel test uses it) for the STATS / BNSUMS column sums.  B > 32: the exact rows of three
images plus a random projection over all rows (tests/conv_check.py); B <= 32: every row exactly.
"""
import ctypes as C
import time

import numpy as np
import pytest
import torch

from oracle import tf_semantics as S
from conv_check import ConvCheck, LinearConv, bf16_round, bf16_ulp, fp8_round, pow2_scale, sums_ratio, E4M3, E5M2

pytestmark = pytest.mark.gpu

CONFIGS = [
    # (label, dtype, mul3, engine switches, batches)
    ("f32", "f32", False, {}, (256, 32, 128, 1)),
    ("f32x3", "f32", True, {}, (32,)),
    ("f32-nowino4", "f32", False, {"winograd4": False}, (32,)),
    ("bf16", "bf16", False, {}, (256, 32)),
    ("fp8", "fp8", False, {}, (256, 32)),
]
SENTINEL = 12288.0          # exact in fp32 and bf16
GUARD = 4096                # elements of sentinel before and after every output buffer
REPORT = []                 # (config, B, layer, role, family, splitk, worst error / gate)
REACHED = {"families": set(), "splitk": 0, "x16": 0, "z16": 0}


def _ops():
    from tumblr_emotions_amd import ops
    return ops


def _fam_names():
    ops = _ops()
    return {v: k[7:] for k, v in vars(ops).items() if k.startswith("DS_FAM_")}


def _copy_plan(src):
    """A private copy of a ds_conv_layer_plan with the on-load fusions cleared and the partial count re-planned."""
    from tumblr_emotions_amd import _lib
    q = _lib.LayerPlanStruct()
    C.memmove(C.addressof(q), C.addressof(src), C.sizeof(q))
    d = q.d
    d.norm_rstd = d.norm_shift = d.mask_rstd = d.mask_shift = None
    d.bnb = d.pool_argmax = None
    _lib.load().ds_conv_plan_set_flags(C.byref(q), d.flags)
    return q


def _harvest(dtype, mul3, switches, B):
    """The plans (copies) of every conv layer after one step of the product engine at batch B (B = 1: input_gradient)."""
    from tumblr_emotions_amd.net import SentimentNet
    net = SentimentNet(mode="image", nb_emotions=15, dtype=dtype)
    eng = net.image
    eng.mul3 = mul3
    for k, v in switches.items():
        setattr(eng, k, v)
    batch = S.synthetic_batch(B, 8, 10, seed=B)
    dev = {k: torch.from_numpy(v).cuda() for k, v in batch.items() if k in ("images", "labels")}
    if B == 1:
        net.input_gradient(dev, 0)
    else:
        net.train_step(dev, 1e-3)
    torch.cuda.synchronize()
    out = []
    for lay in eng.layers:
        for role, pl in (("fwd", lay.fwd), ("dgrad", lay.dgrad)):
            if pl is not None:
                out.append((lay.key.replace("InceptionV1/", ""), role, _copy_plan(pl.p)))
        if lay.wgrad is not None and not lay.fold:
            d = lay.wgrad.d
            out.append((lay.key.replace("InceptionV1/", ""), "wgrad", (d.N, d.H, d.W, d.Cin, d.ldx, d.KH, d.stride, d.Cout)))
    del net, eng
    torch.cuda.empty_cache()
    return out


def _dev_rand(shape, gen, kind):
    if kind == "act":            # post-ReLU like: non-negative, about half exact zeros
        return torch.relu(torch.randn(shape, generator=gen, device="cuda")) * 1.7
    return torch.randn(shape, generator=gen, device="cuda") * 3e-4          # gradients at the network's scale


def _slot(total_ld, c, dtype16):
    """column offset of a c-wide slice in rows of total_ld elements: as far right as 16-element alignment allows"""
    return ((total_ld - c) // 16) * 16


def _gates(p, ops):
    """per-element gate of the family's kernel test and the operand rounding its oracle applies"""
    fam, d = p.family, p.d
    if fam == ops.DS_FAM_FP8D:
        return 1e-4, "fp8"
    if fam == ops.DS_FAM_WINO4H:
        return 5e-4, "bf16"
    if fam == ops.DS_FAM_BF16D:
        return 2e-4, "bf16"
    if fam in (ops.DS_FAM_IGEMM, ops.DS_FAM_STEM, ops.DS_FAM_STEM_POOL) and d.dtype == ops.DS_DTYPE_BF16:
        return 2e-4, "bf16"
    return 2e-4, None


def _sums_gate(p, ops):
    if p.family in (ops.DS_FAM_STEM, ops.DS_FAM_STEM_POOL):
        return 1e-3
    if p.family == ops.DS_FAM_WINO4 and p.splitk > 1:
        return 1e-4 if p.d.flags & ops.DS_EPI_BNSUMS else 1e-3
    return 2e-3


def _replay(p, gen, rng, tag):
    """Run plan p on fresh operands the test owns; returns worst error / gate over every check (asserting each <= 1)."""
    ops = _ops()
    from tumblr_emotions_amd import _lib
    lib = _lib.load()
    st = ops._stream()
    d = p.d
    fam, role = p.family, p.role
    allowed = ops.DS_EPI_STATS | ops.DS_EPI_BNSUMS | ops.DS_EPI_ACCUM
    assert not (d.flags & ~allowed), "%s: epilogue flags %#x not modelled" % (tag, d.flags)
    tol, rounding = _gates(p, ops)
    stem = fam in (ops.DS_FAM_STEM, ops.DS_FAM_STEM_POOL)
    k, wci, wco = p.k, p.w_cin, p.w_cout
    N, H, W = d.N, d.H, d.W
    OH, OW = S.same_pad(H, k, d.stride)[0], S.same_pad(W, k, d.stride)[0]
    dgrad = role == ops.DS_CONV_DGRAD
    # the filter (HWIO; the stem's stored with a zero 4th input channel)
    w = (torch.randn(k, k, wci, wco, generator=gen, device="cuda") * (2.0 / (k * k * min(wci, 3 if stem else wci))) ** 0.5)
    if stem or fam == ops.DS_FAM_STEM_DGRAD:
        w[:, :, 3:] = 0.0
    u = torch.empty(max(p.w_bytes, 4), dtype=torch.uint8, device="cuda")
    wscale = torch.zeros(max(p.wscale_floats, 4), device="cuda")
    _lib.check(lib.ds_conv_prepare_weights(C.byref(p), ops._p(w), ops._p(u), ops._p(wscale), st), "prepare " + tag)
    w_run = w if p.w_bytes == 0 else u
    w64 = w.double().cpu().numpy()
    # input x (fwd: activations [N, H, W, cin] in a row of ldx; dgrad: dz [N, OH', OW', cout] in a row of ldx)
    if stem:
        xg, cin, ldx, x16 = (N, H, W), 3, 3, False
        xbuf = torch.rand(N * H * W * 3, generator=gen, device="cuda") * 2 - 1          # the packed RGB batch in [-1, 1]
        xoff = 0
    else:
        xg = (N, OH, OW) if fam == ops.DS_FAM_STEM_DGRAD else (N, H, W)
        cin, ldx = d.Cin, d.ldx
        x16 = d.x_dtype == ops.DS_DTYPE_BF16
        assert ldx >= cin, tag
        xoff = _slot(ldx, cin, x16)
        rows = xg[0] * xg[1] * xg[2]
        xbuf = _dev_rand((rows, ldx), gen, "grad" if dgrad else "act")
        if x16:
            xbuf = xbuf.to(torch.bfloat16)
        xbuf = torch.cat([xbuf.reshape(-1), torch.zeros(GUARD, dtype=xbuf.dtype, device="cuda")])      # (zero tail: a vector
        # load that runs past the last row stays inside the allocation and does not move max|x|)
    x_seen = xbuf[:xbuf.numel() - (0 if stem else GUARD)].view(-1, ldx)[:, xoff:xoff + cin].double().cpu().numpy().reshape(*xg, cin)
    x_ptr = C.c_void_p(xbuf.data_ptr() + xbuf.element_size() * xoff)
    # the operands the kernel's arithmetic sees
    x_op, w_op = x_seen, w64[:, :, :3] if (stem or fam == ops.DS_FAM_STEM_DGRAD) else w64
    amax = None
    if rounding == "bf16":
        x_op, w_op = bf16_round(x_op), bf16_round(w_op)
    elif rounding == "fp8":
        amax = torch.zeros(ops.AMAX_FLOATS, device="cuda")
        ops.absmax(C.c_void_p(xbuf.data_ptr()), xbuf.numel(), amax, d.x_dtype)       # per-tensor: the whole buffer
        fmt = E4M3 if p.a_format == ops.DS_FP8_E4M3 else E5M2
        torch.cuda.synchronize()
        sx = pow2_scale(ops.amax_value(amax), fmt[0])
        sw = float(wscale[1].item())                       # the filter's scale as the library recorded it
        x_op = fp8_round(x_op * sx, *fmt) / sx
        w_op = fp8_round(w_op * sw, *E4M3) / sw
    if fam == ops.DS_FAM_STEM_DGRAD:
        op = LinearConv("dgrad", w_op, d.stride, H, W)
    elif dgrad:
        op = LinearConv("dgrad", w_op, 1, H, W)
    else:
        op = LinearConv("fwd", w_op, d.stride, H, W)
    chk = ConvCheck(op, x_op, tol, rng)
    # output z (fwd: [N, OH, OW, cout]; dgrad: [N, H, W, cin_w]) in rows of ldz, guards around, sentinel outside the slice
    pooled = fam == ops.DS_FAM_STEM_POOL
    zg = (N, H, W) if (dgrad or fam == ops.DS_FAM_STEM_DGRAD) else (N, OH, OW)
    cout = 3 if fam == ops.DS_FAM_STEM_DGRAD else d.Cout
    ldz = d.ldz
    z16 = d.z_dtype == ops.DS_DTYPE_BF16
    zoff = _slot(ldz, cout, z16)
    zrows = N * (OH // 2) * (OW // 2) if pooled else zg[0] * zg[1] * zg[2]
    zt = torch.bfloat16 if z16 else torch.float32
    zbuf = torch.full((GUARD + zrows * ldz + GUARD,), SENTINEL, dtype=zt, device="cuda")
    zmid = zbuf[GUARD:GUARD + zrows * ldz].view(zrows, ldz)
    prev = None
    if d.flags & ops.DS_EPI_ACCUM:
        prev = torch.randn(zrows, cout, generator=gen, device="cuda") * chk.scale
        zmid[:, zoff:zoff + cout] = prev.to(zt)
        prev = zmid[:, zoff:zoff + cout].double().cpu().numpy()
    z_ptr = C.c_void_p(zbuf.data_ptr() + zbuf.element_size() * (GUARD + zoff))
    io = _lib.ConvIO()
    keep = []
    pivot = None
    if p.partials:
        stats = torch.full((2, cout, p.partials), float("nan"), device="cuda")
        io.stats = stats.data_ptr()
    if d.flags & ops.DS_EPI_STATS or z16:
        pivot = torch.randn(cout, generator=gen, device="cuda") * (0.1 * chk.scale)
        io.pivot = pivot.data_ptr()
    if d.flags & ops.DS_EPI_BNSUMS:
        wino = fam in (ops.DS_FAM_WINO2, ops.DS_FAM_WINO4, ops.DS_FAM_WINO4H)
        ldm = ldz if wino else d.ldmask          # (the Winograd kernels read y with the output's pixel stride)
        assert ldm >= cout, tag
        yb = torch.relu(torch.randn(zrows + 64, ldm, generator=gen, device="cuda")) * \
            (torch.rand(zrows + 64, ldm, generator=gen, device="cuda") < 0.7)
        if d.mask_dtype == ops.DS_DTYPE_BF16:
            yb = yb.to(torch.bfloat16)
        keep.append(yb)
        io.mask = yb.data_ptr() + yb.element_size() * zoff
        y_seen = yb[:zrows, zoff:zoff + cout].double().cpu().numpy()
    if amax is not None:
        io.x_amax = amax.data_ptr()
        io.wscale = wscale.data_ptr()
    if p.ws_bytes:
        ws = torch.full((p.ws_bytes // 4 + 1,), float("nan"), device="cuda")
        keep.append(ws)
        io.ws, io.ws_bytes = ws.data_ptr(), ws.numel() * 4
    _lib.check(lib.ds_conv_run(C.byref(p), x_ptr, ops._p(w_run), z_ptr, C.byref(io), st), "run " + tag)
    torch.cuda.synchronize()
    # nothing written outside the slice
    zb = zbuf.cpu()
    sent = torch.tensor(SENTINEL, dtype=zt)
    assert bool((zb[:GUARD] == sent).all()) and bool((zb[GUARD + zrows * ldz:] == sent).all()), "%s: write outside z" % tag
    zc = zb[GUARD:GUARD + zrows * ldz].view(zrows, ldz)
    outside = torch.cat([zc[:, :zoff], zc[:, zoff + cout:]], 1)
    assert bool((outside == sent).all()), "%s: write into columns outside the slice" % tag
    got = zc[:, zoff:zoff + cout].double().numpy()
    assert np.isfinite(got).all(), tag
    pv = pivot.double().cpu().numpy() if pivot is not None else np.zeros(cout)
    if z16:                         # bf16(z - pivot): compare within one bf16 ulp (+ the fp32 gate)
        got = got + pv
    if prev is not None:
        got = got - prev
    checks = {}
    if pooled:
        # the window maxima of the plain stem launch's z (same MFMA sequence: bit-identical), whose every row is checked
        q = _copy_plan(p)
        q.family = ops.DS_FAM_STEM
        lib.ds_conv_plan_set_flags(C.byref(q), q.d.flags)
        zf = torch.full((N * OH * OW, cout), float("nan"), device="cuda")
        stf = torch.full((2, cout, q.partials), float("nan"), device="cuda")
        io2 = _lib.ConvIO()
        io2.stats, io2.pivot = stf.data_ptr(), pivot.data_ptr()
        _lib.check(lib.ds_conv_run(C.byref(q), x_ptr, ops._p(w_run), ops._p(zf), C.byref(io2), st), "run plain " + tag)
        zp = torch.nn.functional.pad(zf.view(N, OH, OW, cout).permute(0, 3, 1, 2), (0, 1, 0, 1), value=float("-inf"))
        mx = torch.nn.functional.max_pool2d(zp, 3, 2).permute(0, 2, 3, 1).reshape(-1, cout)
        torch.cuda.synchronize()
        assert torch.equal(zc[:, zoff:zoff + cout], mx.cpu()), "%s: pooled maxima differ from the plain launch's" % tag
        got = zf.double().cpu().numpy()
    got = got.reshape(*zg, cout)
    slack = bf16_ulp(chk.ref_imgs - pv) if z16 else None
    checks["rows"] = chk.rows(got, slack)
    if chk.n > len(chk.imgs):
        # (z16: RNE rounding to bf16 is at most half an ulp per element; twice the rms ulp keeps r^T e ~ 7 sigma inside)
        checks["proj"] = chk.projection(got, 2.0 * float(np.sqrt(np.mean(bf16_ulp(got - pv) ** 2))) if z16 else 0.0)
    if d.flags & ops.DS_EPI_STATS:
        sg = _sums_gate(p, ops)
        s = stats.double().cpu().numpy().sum(2)
        u = got.reshape(-1, cout) - pv
        checks["stats"] = max(sums_ratio(s[0], u.sum(0), sg), sums_ratio(s[1], (u * u).sum(0), sg))
        Mz = u.shape[0]
        checks["stats~ref"] = sums_ratio(s[0], chk.column_sums() - Mz * pv, sg)
    if d.flags & ops.DS_EPI_BNSUMS:
        sg = _sums_gate(p, ops)
        s = stats.double().cpu().numpy().sum(2)
        dxf = zc[:, zoff:zoff + cout].double().numpy()
        gm = dxf * (y_seen > 0)
        checks["bnsums"] = max(sums_ratio(s[0], gm.sum(0), sg), sums_ratio(s[1], (gm * y_seen).sum(0), sg))
    for name, r in checks.items():
        assert r <= 1.0, "%s: %s check at %.2f x its gate (tol %.0e)" % (tag, name, r, tol)
    REACHED["families"].add(fam)
    REACHED["splitk"] += int(fam == ops.DS_FAM_WINO4 and p.splitk > 1)
    REACHED["x16"] += int(x16 and p.x16_ok)
    REACHED["z16"] += int(z16)
    return max(checks.values())


def _replay_wgrad(shape, gen, rng, tag):
    """Mixed_5c's (or any trainable layer's) Conv2DBackpropFilter: ds_conv_wgrad against S.conv2d_same_bwd_filter, 5e-4."""
    ops = _ops()
    N, H, W, Cin, ldx, k, s, Cout = shape
    ldx = max(ldx, Cin)
    xoff = _slot(ldx, Cin, False)
    x = _dev_rand((N * H * W, ldx), gen, "act")
    OH, OW = S.same_pad(H, k, s)[0], S.same_pad(W, k, s)[0]
    dz = torch.randn(N * OH * OW, Cout, generator=gen, device="cuda") * 3e-4
    plan = ops.WgradPlan(N, H, W, Cin, ldx, k, k, s, Cout, Cout)
    ws = torch.empty(max(plan.ws_bytes // 4, 4), device="cuda")
    dw = torch.full((k * k * Cin * Cout,), float("nan"), device="cuda")
    plan.run(C.c_void_p(x.data_ptr() + 4 * xoff), ops._p(dz), ops._p(dw), ops._p(ws), plan.ws_bytes)
    torch.cuda.synchronize()
    x64 = x[:, xoff:xoff + Cin].double().cpu().numpy().reshape(N, H, W, Cin)
    ref = S.conv2d_same_bwd_filter(x64, dz.double().cpu().numpy().reshape(N, OH, OW, Cout), (k, k, Cin, Cout), s)
    r = float(np.abs(dw.double().cpu().numpy().reshape(ref.shape) - ref).max() / (5e-4 * np.abs(ref).max()))
    assert r <= 1.0, "%s: wgrad at %.2f x its gate" % (tag, r)
    return r


def _key(layer, role, p):
    return (layer, role, p.family, p.splitk) if not isinstance(p, tuple) else (layer, role, "wgrad")


@pytest.mark.parametrize("cfg", CONFIGS, ids=[c[0] for c in CONFIGS])
def test_every_conv_plan_of_the_image_engine_matches_fp64(cfg):
    label, dtype, mul3, switches, batches = cfg
    fam = _fam_names()
    t0 = time.time()
    seen = {}
    for B in batches:
        plans = _harvest(dtype, mul3, switches, B)
        gen = torch.Generator(device="cuda")
        gen.manual_seed(1000 + B)
        rng = np.random.RandomState(B)
        for layer, role, p in plans:
            key = _key(layer, role, p)
            if B == 128 and key in seen:            # B = 128: only the launches neither 256 nor 32 made
                continue
            seen[key] = B
            tag = "%s B=%d %s %s" % (label, B, layer, role)
            if role == "wgrad":
                if dtype != "f32" or B == 1:
                    continue
                r = _replay_wgrad(p, gen, rng, tag)
                REPORT.append((label, B, layer, role, "WGRAD", 1, r))
                continue
            r = _replay(p, gen, rng, tag)
            REPORT.append((label, B, layer, role, fam[p.family], p.splitk, r))
    print("\n%s: %d launches in %.1f s" % (label, sum(1 for r in REPORT if r[0] == label), time.time() - t0))
    for row in REPORT:
        if row[0] == label:
            print("  %-12s B=%-3d %-48s %-5s %-9s splitk=%d  %.3f" % row)


def test_the_configurations_reach_every_family_of_the_tower():
    """Run after the replays above (same module): the configurations together reach every family ds_conv_plan returns for
    the tower, at least one split-K F(4x4) plan, one x16_ok plan fed 16-bit input and one z16 output."""
    ops = _ops()
    if not REPORT:
        pytest.skip("needs the replays of this module in the same session")      # (only when selected alone)
    want = {ops.DS_FAM_IGEMM, ops.DS_FAM_WINO2, ops.DS_FAM_WINO4, ops.DS_FAM_STEM, ops.DS_FAM_BF16D, ops.DS_FAM_FP8D,
            ops.DS_FAM_F32X3, ops.DS_FAM_WINO4H, ops.DS_FAM_STEM_POOL, ops.DS_FAM_STEM_DGRAD}
    fam = _fam_names()
    assert REACHED["families"] == want, sorted(fam[f] for f in want - REACHED["families"])
    assert REACHED["splitk"] >= 1 and REACHED["x16"] >= 1 and REACHED["z16"] >= 1, REACHED
