"""Records tests/golden/igemm_plan_table.json: what the host-side plan of the conv library answers for every conv / GEMM
shape the suite knows -- no device needed, nothing is launched.

    python tests/golden/make_igemm_plan_table.py PRODUCT_LIB TUNING_LIB      # libds_kernels.so, libds_kernels_tuning.so

The fixture pins the answers of the commit it was recorded from (the two libraries of the commit BEFORE the host dispatch of
conv_igemm.hip was rewritten); tests/test_igemm_plan_table_cpu.py asks the tree's libraries the same questions.

Rows: every shape of test_fused_inference_cpu.inception_stride1_shapes() (forward and Conv2DBackpropInput) and the toy table of
test_conv_layers_cpu.SHAPES at N in {1, 8, 32, 64} (the toy rows also at their own N), the packed-RGB stem (direct and folded
into the implicit GEMM) at N in {1, 8, 16}, and the head GEMMs of tests/head_ref.py (JOINT_CASES / TEXT_CASES at their own
batch, plain and with the split-K slices ops.head_gemm_plan gives them).  Every launch stays at <= 2048 row tiles, so no answer
depends on the occupancy query, which fails without a device (asserted per row).

Per row, through ds_conv_plan for f32 / bf16 / fp8 / f32x3: the return code, family, partials, splitk, ws_bytes, w_bytes, x16_ok
and what ds_conv_plan_enable_bnsums / _enable_pool3 / _enable_bn_relu / _norm_supported / _bnb_supported answer (with the
partial counts they leave in the plan); through a raw ds_conv_desc: the five ds_conv_igemm_* answers without
flags and with DS_EPI_STATS.  Of the product library the raw answers and the f32 plan are stored in full and the bf16 / fp8 /
f32x3 plans as one sha256 prefix each.  The tuning library answers the same under ds_debug_conv_set_wide 0 / 1 / 2, set_path
1 / 3 (the two families it pins) and set_tile (1,1) .. (2,6); of those, one sha256 prefix
per shape (all its N) is stored, in the order of shapes().  That keeps the file under 200 KB."""
import ctypes as C
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)

from tumblr_emotions_amd import _lib as L      # noqa: E402  (constants, ctypes mirrors and signatures only)

FIXTURE = os.path.join(HERE, "igemm_plan_table.json")
ARITHS = (L.DS_ARITH_F32, L.DS_ARITH_BF16, L.DS_ARITH_FP8, L.DS_ARITH_F32X3)
BATCHES, STEM_BATCHES = (1, 8, 32, 64), (1, 8, 16)
TUNING_CONFIGS = ([("default", ())] + [("wide%d" % m, (("ds_debug_conv_set_wide", (m,)),)) for m in (0, 1, 2)] +
                  [("path%d" % m, (("ds_debug_conv_set_path", (m,)),)) for m in (1, 3)] +
                  [("tile%d,%d" % (mt, nt), (("ds_debug_conv_set_tile", (mt, nt)),)) for mt in (1, 2) for nt in range(1, 7)])


def open_library(path, tuning=False):
    lib = C.CDLL(path)
    L._bind(lib, L.SIGNATURES)
    if tuning:
        L._bind(lib, L.DEBUG_SIGNATURES)
    return lib


def same_pad(n, k, s):
    out = -(-n // s)
    return out, max((out - 1) * s + k - n, 0) // 2


def shapes():
    """[(shape key, [row, ..])]; a row is (role, options, N, H, W, w_cin, w_cout, k, stride, splits)."""
    from head_ref import JOINT_CASES, TEXT_CASES, plan_splits
    from test_conv_layers_cpu import SHAPES
    from test_fused_inference_cpu import inception_stride1_shapes
    out = []
    for hw, ci, co, k in inception_stride1_shapes():
        for role in (L.DS_CONV_FWD, L.DS_CONV_DGRAD):
            out.append(("inception %d %d %d %d role%d" % (hw, ci, co, k, role),
                        [(role, 0, N, hw, hw, ci, co, k, 1, 1) for N in BATCHES]))
    for name, opt in (("stem", L.DS_PLAN_PACKED_RGB), ("stem folded", L.DS_PLAN_PACKED_RGB | L.DS_PLAN_NO_STEM_DIRECT)):
        out.append((name, [(L.DS_CONV_FWD, opt, N, 224, 224, 4, 64, 7, 2, 1) for N in STEM_BATCHES]))
    gemms = set()
    for B, im, tx, fc, nc in JOINT_CASES:
        gemms |= {(B, im, fc), (B, tx, fc), (B, fc, nc), (B, nc, fc), (B, fc, im), (B, fc, tx)}
    for B, H, nc in TEXT_CASES:
        gemms |= {(B, H, nc), (B, nc, H)}
    for K, N in sorted({(K, N) for _, K, N in gemms}):
        rows = []
        for M in sorted({M for M, k, n in gemms if (k, n) == (K, N)}):
            for splits in sorted({1, plan_splits(M, K) or 1}):
                rows.append((L.DS_CONV_FWD, 0, M, 1, 1, K, N, 1, 1, splits))
        out.append(("head %d %d" % (K, N), rows))
    for role, N0, H, W, ci, co, k, s in SHAPES:
        r = L.DS_CONV_FWD if role == "fwd" else L.DS_CONV_DGRAD
        for opt in (0, L.DS_PLAN_PACKED_RGB) if k == 7 else (0,):
            out.append(("toy %s %d %d %d %d %d %d opt%d" % (role, H, W, ci, co, k, s, opt),
                        [(r, opt, N, H, W, ci, co, k, s, 1) for N in sorted(set(BATCHES) | {N0})]))
    return out


def raw_desc(row):
    """The ds_conv_desc ops.ConvPlan / ops.gemm_plan would build for the row's launch (weights read in place)."""
    role, _, N, H, W, w_cin, w_cout, k, s, splits = row
    dgrad = role == L.DS_CONV_DGRAD
    cin, cout = (w_cout, w_cin) if dgrad else (w_cin, w_cout)
    d = L.ConvDesc()
    d.N, d.H, d.W, d.Cin, d.ldx, d.KH, d.KW, d.stride, d.Cout, d.ldz = N, H, W, cin, cin, k, k, s, cout, cout
    (d.OH, d.pad_t), (d.OW, d.pad_l) = same_pad(H, k, s), same_pad(W, k, s)
    d.w_tap_stride, d.w_n_stride, d.w_k_stride, d.flip = w_cin * w_cout, (w_cout if dgrad else 1), (1 if dgrad else w_cout), int(dgrad)
    d.splits, d.z_split_stride, d.dtype = splits, (N * d.OH * d.OW * cout if splits > 1 else 0), L.DS_DTYPE_F32
    return d


def digest(obj):
    return hashlib.sha256(json.dumps(obj).encode()).hexdigest()[:8]


def answers(lib, row):
    """What is recorded for one row: [the raw descriptor's answers, the f32 plan's, the bf16 / fp8 / f32x3 plans']."""
    role, options, N, H, W, w_cin, w_cout, k, s, splits = row
    d = raw_desc(row)
    assert -(-(N * d.OH * d.OW) // 128) <= 2048, ("more than 2048 row tiles: the answer would depend on the device", row)
    out = []
    for flags in (0, L.DS_EPI_STATS):
        d.flags = flags
        out += [lib.ds_conv_igemm_partials(C.byref(d)), lib.ds_conv_igemm_bnsums_supported(C.byref(d)),
                lib.ds_conv_igemm_norm_supported(C.byref(d)), lib.ds_conv_igemm_pool3_supported(C.byref(d)),
                lib.ds_conv_igemm_bnb_supported(C.byref(d))]
    dgrad = role == L.DS_CONV_DGRAD
    ldx, ldz = (w_cout, w_cin) if dgrad else (w_cin, w_cout)
    if options & L.DS_PLAN_PACKED_RGB:
        ldx, ldz = (64, 3) if dgrad else (3, w_cout)

    def plan(arith, flags):
        p = L.LayerPlanStruct()
        rc = lib.ds_conv_plan(C.byref(p), role, arith, options, N, H, W, w_cin, w_cout, k, s, ldx, ldz, flags)
        if rc == 0 and splits > 1:      # (ops.SplitGemm: the slices are set on the descriptor)
            p.d.splits, p.d.z_split_stride = splits, N * p.d.OH * p.d.OW * p.d.Cout
        return rc, p

    blocks = [out]
    for arith in ARITHS:
        rc, p = plan(arith, 0 if dgrad or splits > 1 else L.DS_EPI_STATS)
        out = [rc]
        blocks.append(out)
        if rc != 0:
            continue
        out += [p.family, p.partials, p.d.partials, p.splitk, p.ws_bytes, p.w_bytes, p.x16_ok,
                lib.ds_conv_plan_norm_supported(C.byref(p)), lib.ds_conv_plan_bnb_supported(C.byref(p))]
        q = L.LayerPlanStruct.from_buffer_copy(p)
        out += [lib.ds_conv_plan_enable_bnsums(C.byref(q), ldz), q.d.flags, q.partials, q.d.partials]
        q = L.LayerPlanStruct.from_buffer_copy(p)
        out += [lib.ds_conv_plan_enable_pool3(C.byref(q), C.c_void_p(4096)), q.partials, q.d.partials]
        out += [lib.ds_conv_plan_norm_supported(C.byref(q))]
        out += [lib.ds_conv_plan_set_flags(C.byref(q), 0), lib.ds_conv_plan_enable_bn_relu(C.byref(q)), q.d.flags]
        rc, q = plan(arith, 0)
        out += [lib.ds_conv_plan_enable_bn_relu(C.byref(q)), q.d.flags, q.partials, q.d.partials]
    return blocks


def product_rows(lib):
    """[[shape key, [[row, raw answers, f32 plan, digest of the bf16 plan, .. fp8, .. f32x3], ..]], ..]"""
    return [[key, [[list(row)] + answers(lib, row)[:2] + [digest(b) for b in answers(lib, row)[2:]] for row in rows]]
            for key, rows in shapes()]


def tuning_digests(tuning):
    """{config: [sha256 prefix of a shape's answers under that config, in the order of shapes()]}; the switches are put back."""
    out = {}
    try:
        for name, calls in TUNING_CONFIGS:
            for fn, args in calls:
                assert getattr(tuning, fn)(*args) == 0, (fn, args)
            out[name] = [digest([answers(tuning, row) for row in rows]) for _, rows in shapes()]
            reset(tuning)
    finally:
        reset(tuning)
    return out


def reset(tuning):
    tuning.ds_debug_conv_set_wide(1)
    tuning.ds_debug_conv_set_path(0)
    tuning.ds_debug_conv_set_tile(0, 0)


def main():
    product, tuning = open_library(sys.argv[1]), open_library(sys.argv[2], tuning=True)
    rows, digests = product_rows(product), tuning_digests(tuning)
    with open(FIXTURE, "w") as f:
        f.write('{"rows": [\n' + ",\n".join(json.dumps(r, separators=(",", ":")) for r in rows) + '\n],\n"tuning": {\n' +
                ",\n".join('%s: %s' % (json.dumps(k), json.dumps(v, separators=(",", ":"))) for k, v in digests.items()) + "\n}}\n")
    print("%s: %d rows of %d shapes, %d tuning configurations, %d bytes" %
          (FIXTURE, sum(len(r[1]) for r in rows), len(rows), len(digests), os.path.getsize(FIXTURE)))


if __name__ == "__main__":
    main()
