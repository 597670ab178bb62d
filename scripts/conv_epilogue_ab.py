#!/usr/bin/env python
"""A/B of the conv kernels' epilogues (csrc/conv_epilogue.h) between two builds of the library.

    DS_LIB=<a libds_kernels_tuning.so> python scripts/conv_epilogue_ab.py run OUT.json [--no-digest] [--no-time] [--small] [--only=SUBSTRING]
    python scripts/conv_epilogue_ab.py compare OUT.json PARENT.json TREE.json [PARENT2.json TREE2.json ...]

`run` walks a fixed, seeded case list -- each of the six kernels with every epilogue its entry point accepts -- and writes,
per case, a SHA-256 of every output buffer and an event-timed median.  Each combination runs at the smallest shape that
reaches every guard (1x1, M = 165, Cin = 32, Cout = 40, ldz = ldmask = 48: in the second row tile wave 0 is full, wave 1
has 5 rows, waves 2-3 none, and column block 1 is partial), one 3x3 case per kernel that takes 3x3, and the B = 256 1x1
shapes of scripts/wide_epi_bench.py for the timing.  `compare`: equal digests on the cases both builds have, and the second build's median per timed case
inside the range of the first build's window medians."""
import ast
import hashlib
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import _tuning  # noqa: F401,E402  (the -DDS_TUNING library: ds_debug_* switches pin the kernel)

_HERE = os.path.dirname(os.path.abspath(__file__))
SHAPES = next(ast.literal_eval(n.value) for n in ast.parse(open(os.path.join(_HERE, "wide_epi_bench.py")).read()).body
              if isinstance(n, ast.Assign) and getattr(n.targets[0], "id", "") == "SHAPES")
SMALL = (165, 32, 40, 48)          # M, K, N, ldz = ldmask


def compare(out, files):
    runs = [json.load(open(f)) for f in files]
    a, b = runs[0::2], runs[1::2]
    res = {"digest_mismatch": [], "only_in_first": [], "slower": [], "timed_cases": 0, "cases": len(a[0]["cases"])}
    for name, ca in a[0]["cases"].items():
        cb = b[0]["cases"].get(name)
        if cb is None:          # a case of a kernel the second build no longer has
            res["only_in_first"].append(name)
            continue
        if ca.get("sha256") != cb.get("sha256") or ca.get("skipped") != cb.get("skipped"):
            res["digest_mismatch"].append(name)
        if not ca.get("timed") or ca.get("skipped") or "us" not in ca:
            continue
        res["timed_cases"] += 1
        ta = [r["cases"][name]["us"] for r in a]
        tb = sorted(r["cases"][name]["us"] for r in b)
        med = tb[len(tb) // 2] if len(tb) % 2 else 0.5 * (tb[len(tb) // 2 - 1] + tb[len(tb) // 2])
        if med > max(ta):
            res["slower"].append({"case": name, "first": ta, "second": tb})
    both = set(a[0]["cases"]) & set(b[0]["cases"])
    tot = lambda rs: [round(sum(c["us"] for n, c in r["cases"].items() if n in both and c.get("timed") and "us" in c), 1) for r in rs]
    res["total_us_first"], res["total_us_second"] = tot(a), tot(b)
    res["libs"] = [r["lib"] for r in runs]
    json.dump(res, open(out, "w"), indent=1)
    print(json.dumps({k: (v if not isinstance(v, list) or len(v) < 12 else v[:12] + ["..."]) for k, v in res.items()}, indent=1))
    return 0 if not res["digest_mismatch"] else 1


def main():
    if sys.argv[1] == "compare":
        return compare(sys.argv[2], sys.argv[3:])
    import torch
    from tumblr_emotions_amd import _lib, ops
    out, digest, timing, small_only = sys.argv[2], "--no-digest" not in sys.argv, "--no-time" not in sys.argv, "--small" in sys.argv
    only = next((a[7:] for a in sys.argv if a.startswith("--only=")), "")
    lib = _lib.load()
    E = ops
    dev = "cuda"
    results = {}

    def rnd(*shape, scale=1.0):
        return torch.randn(*shape, device=dev) * scale

    def pin(path, wide, mt, nt):
        assert lib.ds_debug_conv_set_path(path) == 0 and lib.ds_debug_conv_set_wide(wide) == 0 and lib.ds_debug_conv_set_tile(mt, nt) == 0

    def sha(t):
        return hashlib.sha256(t.contiguous().view(torch.uint8).cpu().numpy()).hexdigest()

    def record(name, timed, build):
        """build() -> (launch, reset, [(label, output tensor)], what else must stay alive), or None when the library does not
        carry the combination for the shape."""
        if only not in name:
            return
        torch.manual_seed(int(hashlib.sha256(name.encode()).hexdigest()[:7], 16))
        why = "not carried for this shape"
        try:
            made = build()
        except (RuntimeError, ValueError) as e:          # refused by the entry point: both builds must refuse it
            made, why = None, str(e)[:160]
        if made is None:
            results[name] = {"skipped": why, "timed": timed}
            return
        launch, reset, outs, _keep = made
        r = {"timed": timed}
        reset()
        launch()
        torch.cuda.synchronize()
        if digest:
            r["sha256"] = {label: sha(t) for label, t in outs}
        for _ in range(2 if timing else 0):
            launch()
        samples = []
        for _ in range(7 if timing else 0):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(3):
                launch()
            e1.record()
            torch.cuda.synchronize()
            samples.append(e0.elapsed_time(e1) / 3 * 1e3)
        if timing:
            r["us"] = round(sorted(samples)[3], 2)
        results[name] = r

    # ---- the three tile kernels, through ds_conv_igemm ------------------------------------------------------------------------
    TILE = {"0": 0, "BIAS": E.DS_EPI_BIAS, "BIAS|RELU": E.DS_EPI_BIAS | E.DS_EPI_RELU, "ACCUM": E.DS_EPI_ACCUM,
            "MASK": E.DS_EPI_MASK, "STATS+pivot": E.DS_EPI_STATS}

    def tile_case(kern, combo, geom, mt=1):
        """geom: (N, H, W, Cin, Cout, k, ldz)"""
        N, H, W, K, Nc, k, ld = geom
        path, dtype = {"lds": (1, E.DS_DTYPE_F32), "glds": (3, E.DS_DTYPE_F32), "bf16t": (0, E.DS_DTYPE_BF16)}[kern]

        def build():
            pin(path, 0, mt, 2)
            x, w = rnd(N, H, W, K), rnd(k, k, K, Nc, scale=0.1)
            if combo == "BNR":
                plan = E.LayerPlan(E.DS_CONV_FWD, E.DS_ARITH_F32, 0, N, H, W, K, Nc, k, 1, K, ld, 0)
                q = plan.bn_relu_variant(ld) if plan.family == E.DS_FAM_IGEMM else None
                if q is None:
                    return None
                z, sc, sh = torch.empty(N * H * W, ld, device=dev), torch.rand(Nc, device=dev) + 0.1, rnd(Nc)
                return (lambda: q.run_bn_relu(E._p(x), E._p(w), E._p(z), sc.data_ptr(), sh.data_ptr())), (lambda: z.fill_(-7.0)), [("z", z)], None
            flags = TILE[combo]
            plan = E.ConvPlan(N, H, W, K, K, k, k, 1, Nc, ld, K * Nc, 1, Nc, flags=flags, ldmask=ld, dtype=dtype)
            M = plan.M
            z, prev = torch.empty(M, ld, device=dev), rnd(M, ld)
            bias, mask, pivot = rnd(Nc), rnd(M, ld), rnd(Nc, scale=0.2)
            stats = torch.zeros(2 * Nc * max(plan.partials, 1) + 16, device=dev)
            run = lambda: plan.run(E._p(x), E._p(w), E._p(z), bias=E._p(bias), mask=E._p(mask), stats=E._p(stats),
                                   pivot=E._p(pivot) if flags & E.DS_EPI_STATS else None)
            return run, (lambda: z.copy_(prev)), [("z", z), ("stats", stats)], None
        return build

    # ---- the wide 1x1 kernel -------------------------------------------------------------------------------------------------
    def wide_case(combo, M, K, Nc, ld):
        def build():
            pin(0, 2, 0, 0)
            x = rnd(M, K)
            if combo == "BNR":
                w = rnd(K, Nc, scale=0.1)
                plan = E.LayerPlan(E.DS_CONV_FWD, E.DS_ARITH_F32, 0, 1, M, 1, K, Nc, 1, 1, K, ld, 0)
                if plan.family != E.DS_FAM_IGEMM:
                    return None
                z = torch.empty(M, ld, device=dev)
                q = plan.bn_relu_variant(ld)
                if q is None:
                    return None
                sc, sh = torch.rand(Nc, device=dev) + 0.1, rnd(Nc)
                return (lambda: q.run_bn_relu(E._p(x), E._p(w), E._p(z), sc.data_ptr(), sh.data_ptr())), (lambda: z.fill_(-7.0)), [("z", z)], None
            if combo in ("0", "STATS+pivot"):          # forward: n-contiguous weights
                flags = E.DS_EPI_STATS if combo != "0" else 0
                w = rnd(K, Nc, scale=0.1)
                plan = E.ConvPlan(M, 1, 1, K, K, 1, 1, 1, Nc, ld, 0, 1, Nc, flags=flags, pad_t=0, pad_l=0, OH=1, OW=1)
            else:                                      # dgrad: k-contiguous weights
                flags = E.DS_EPI_ACCUM
                w = rnd(Nc, K, scale=0.1)
                plan = E.gemm_plan(M, K, Nc, K, ld, K, transposed_w=True, flags=flags)
            z, prev, y, pivot = torch.empty(M, ld, device=dev), rnd(M, ld), rnd(M, ld), rnd(Nc, scale=0.2)
            mr, ms = torch.rand(Nc, device=dev) + 0.5, rnd(Nc, scale=0.3)
            if "BNSUMS" in combo:
                if not plan.enable_bnsums(ld):
                    return None
                if "mask_rstd" in combo:
                    plan.d.mask_rstd, plan.d.mask_shift = mr.data_ptr(), ms.data_ptr()
                else:
                    y.clamp_(min=0.0)
            stats = torch.zeros(2 * Nc * max(plan.partials, 1) + 16, device=dev)
            run = lambda: plan.run(E._p(x), E._p(w), E._p(z), mask=E._p(y), stats=E._p(stats), pivot=E._p(pivot) if flags & E.DS_EPI_STATS else None)
            return run, (lambda: z.copy_(prev)), [("z", z), ("stats", stats)], (mr, ms)
        return build

    def pool_case(N, H, W, K, Nc, ld):
        """gemm_wide_kernel<.., POOL>: the 3x3 / 1 max pool on load, whose 32-row blocks end with a wave's last real row (Mw)."""
        def build():
            pin(0, 2, 0, 0)
            x, w = rnd(N, H, W, K), rnd(K, Nc, scale=0.1)
            plan = E.LayerPlan(E.DS_CONV_FWD, E.DS_ARITH_F32, 0, N, H, W, K, Nc, 1, 1, K, ld, E.DS_EPI_STATS)
            argmax = torch.zeros(N * H * W, K, dtype=torch.uint8, device=dev)
            if plan.family != E.DS_FAM_IGEMM or not plan.enable_pool3(argmax):
                return None
            z, pivot = torch.empty(N * H * W, ld, device=dev), rnd(Nc, scale=0.2)
            stats = torch.zeros(2 * Nc * max(plan.partials, 1) + 16, device=dev)
            run = lambda: plan.run(E._p(x), E._p(w), E._p(z), stats=E._p(stats), pivot=E._p(pivot))
            return run, (lambda: z.fill_(-7.0)), [("z", z), ("stats", stats), ("argmax", argmax)], None
        return build

    # ---- the register-direct bf16 / f32x3 / fp8 kernels ----------------------------------------------------------------------
    def rowdirect_case(kern, combo, geom):
        N, H, W, K, Nc, k, ld = geom

        def build():
            x, w = rnd(N, H, W, K), rnd(k, k, K, Nc, scale=0.1)
            flags = {"0": 0, "STATS+pivot": E.DS_EPI_STATS, "z16": E.DS_EPI_STATS, "ACCUM": E.DS_EPI_ACCUM}.get(combo, E.DS_EPI_ACCUM | E.DS_EPI_BNSUMS)
            grad = bool(flags & E.DS_EPI_ACCUM)
            if kern == "bf16d":
                plan = E.Bf16Plan(N, H, W, K, K, k, 1, Nc, ld, flags=flags)
                wq = torch.empty(E.weights_bf16_bytes(K, Nc, k * k, False), dtype=torch.uint8, device=dev)
                E.weights_to_bf16(E._p(w), wq, K, Nc, k * k, False)
            elif kern == "x3":
                plan = E.F32x3Plan(N, H, W, K, K, k, 1, Nc, ld, flags=flags)
                wq = torch.empty(E.weights_f32x3_bytes(K, Nc, k * k, False), dtype=torch.uint8, device=dev)
                E.weights_to_f32x3(E._p(w), wq, K, Nc, k * k, False)
            else:
                plan = E.Fp8Plan(N, H, W, K, K, k, 1, Nc, ld, flags=flags, a_format=E.DS_FP8_E5M2 if grad else E.DS_FP8_E4M3)
                wq = torch.empty(E.weights_fp8_bytes(K, Nc, k * k, False), dtype=torch.uint8, device=dev)
                ws, amax = torch.zeros(E.WSCALE_FLOATS, device=dev), torch.zeros(E.AMAX_FLOATS, device=dev)
                E.weights_to_fp8(E._p(w), wq, ws, K, Nc, k * k, False)
                E.absmax(x, x.numel(), amax)
            M = plan.M
            z16, m16 = combo == "z16", combo == "m16"
            z = torch.empty(M, ld, device=dev, dtype=torch.bfloat16 if z16 else torch.float32)
            prev = rnd(M, ld).to(z.dtype)
            y = rnd(M, ld)
            mr, ms = torch.rand(Nc, device=dev) + 0.5, rnd(Nc, scale=0.3)
            if "mask_rstd" in combo:
                plan.d.mask_rstd, plan.d.mask_shift = mr.data_ptr(), ms.data_ptr()
            else:
                y.clamp_(min=0.0)
            if m16:
                y = y.to(torch.bfloat16)
            plan.d.ldmask, plan.d.mask_dtype = ld, E.DS_DTYPE_BF16 if m16 else E.DS_DTYPE_F32
            plan.d.z_dtype = E.DS_DTYPE_BF16 if z16 else E.DS_DTYPE_F32
            pivot = rnd(Nc, scale=0.2)
            stats = torch.zeros(2 * Nc * ((M + 127) // 128) + 16, device=dev)
            kw = dict(stats=E._p(stats), pivot=E._p(pivot) if flags & E.DS_EPI_STATS else None, mask=E._p(y))
            if kern == "fp8d":
                kw.update(x_amax=E._p(amax), wscale=E._p(ws))
            run = lambda: plan.run(E._p(x), E._p(wq), E._p(z), **kw)
            return run, (lambda: z.copy_(prev)), [("z", z), ("stats", stats)], (mr, ms)
        return build

    WIDE = ["0", "STATS+pivot", "ACCUM", "ACCUM|BNSUMS", "ACCUM|BNSUMS+mask_rstd", "BNR"]
    ROWD = {"bf16d": ["0", "STATS+pivot", "ACCUM", "ACCUM|BNSUMS", "m16", "z16"],
            "x3": ["0", "STATS+pivot", "ACCUM|BNSUMS", "ACCUM|BNSUMS+mask_rstd"],
            "fp8d": ["0", "STATS+pivot", "ACCUM", "ACCUM|BNSUMS", "m16", "z16"]}
    TILES = {"lds": list(TILE) + ["BNR"], "glds": list(TILE) + ["BNR"], "bf16t": list(TILE)}
    g3 = (1, 8, 8, 16, 40, 3, 48)
    M, K, Nc, ld = SMALL
    try:
        for kern, combos in TILES.items():
            for combo in combos:
                record("small/%s/%s" % (kern, combo), False, tile_case(kern, combo, (M, 1, 1, K, Nc, 1, ld)))
                if kern == "lds" and combo != "BNR":          # the 256-row tile: the MT loop
                    record("small/%s-mt2/%s" % (kern, combo), False, tile_case(kern, combo, (M, 1, 1, K, Nc, 1, ld), mt=2))
            record("3x3/%s/STATS+pivot" % kern, False, tile_case(kern, "STATS+pivot", g3))
        for combo in WIDE:
            record("small/wide/%s" % combo, False, wide_case(combo, M, K, Nc, ld))
        record("small/wide/POOL+STATS", False, pool_case(3, 7, 7, 32, Nc, ld))          # 28-pixel blocks, a surplus wave
        record("small/wide/POOL+STATS-14", False, pool_case(2, 14, 14, 32, Nc, ld))
        pin(0, 1, 0, 0)
        for kern, combos in ROWD.items():
            for combo in combos:
                record("small/%s/%s" % (kern, combo), False, rowdirect_case(kern, combo, (M, 1, 1, K, Nc, 1, ld)))
            record("3x3/%s/STATS+pivot" % kern, False, rowdirect_case(kern, "STATS+pivot", g3))
        for (hw, ci, co) in ([] if small_only else SHAPES):
            Mb = 256 * hw * hw
            fwd, dgr = (Mb, ci, co, co), (Mb, co, ci, ci)              # accumulate / sums combinations run the dgrad's shape
            tag = "b256/%dx%d_%d_%d" % (hw, hw, ci, co)
            for kern, combos in TILES.items():
                for combo in combos:
                    m_, k_, n_, l_ = dgr if combo == "ACCUM" else fwd
                    record("%s/%s/%s" % (tag, kern, combo), True, tile_case(kern, combo, (m_, 1, 1, k_, n_, 1, l_)))
            for combo in WIDE:
                record("%s/wide/%s" % (tag, combo), True, wide_case(combo, *(dgr if "ACCUM" in combo else fwd)))
            pin(0, 1, 0, 0)
            for kern, combos in ROWD.items():
                for combo in combos:
                    m_, k_, n_, l_ = fwd if combo in ("0", "STATS+pivot", "z16") else dgr
                    record("%s/%s/%s" % (tag, kern, combo), True, rowdirect_case(kern, combo, (m_, 1, 1, k_, n_, 1, l_)))
            print("%s done (%d cases so far)" % (tag, len(results)), flush=True)
    finally:
        pin(0, 1, 0, 0)
        json.dump({"lib": os.environ.get("DS_LIB"), "digest": digest, "cases": results}, open(out, "w"), indent=1)
    print("%s: %d cases, %d skipped" % (out, len(results), sum(1 for r in results.values() if "skipped" in r)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
