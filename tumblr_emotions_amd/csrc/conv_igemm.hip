// Implicit-GEMM convolution / GEMM on the fp32 matrix cores of gfx950 (v_mfma_f32_32x32x2_f32).
//
// Replaces slim.conv2d's Conv2D, its Conv2DBackpropInput, and every tf.matmul on the Deep
// Sentiment path (reference call sites: see include/ds_kernels.h).  Design notes:
//   * A operand = NHWC activations, gathered tap by tap (no im2col buffer); K-tile = 16
//     channels of one tap, so a row of the A tile is 64 contiguous bytes of one input pixel.
//   * B operand = the TF HWIO weight tensor read in place through (tap, n, k) strides: forward
//     convs see it n-contiguous (staged [k][n] in LDS, fragments read with conflict-free
//     ds_read_b32), dgrad sees it k-contiguous with the tap order flipped (staged [n][k], fragments
//     read with ds_read_b128 like A).  Nothing is ever re-packed.
//   * all global reads are SRD buffer loads (buffer_load_dwordx4 ... offen): padding pixels, the K
//     tail and rows/columns past the tensor get an out-of-range offset and the hardware returns
//     zeros -- no branches and no selects in the main loop, so a K-tile's loads issue back to back,
//     stay in flight under the MFMAs of the current tile and are waited for only at the LDS store.
//   * 4 waves per workgroup stacked along M; each wave owns (MT*32) rows x all BN = NT*32 columns,
//     so the tile width is chosen per layer from NT = 1..6 to fit Cout with little padding.
//   * launch geometry (choose): one workgroup per row tile up to 2048 row tiles; above that the
//     workgroups are persistent over row tiles (grid.x a multiple of 8 so that all column tiles of
//     a row tile, which share the A rows, land on the same XCD/L2) with the K-loop pipeline running
//     across tiles.  BatchNorm column statistics are accumulated in registers and emitted once per
//     workgroup either way.
//   * fp32 MFMA is an exact k-ordered fmaf chain (cdna_hip_programming.md section 3), so results
//     match a scalar fp32 reference to rounding.
#include <stdlib.h>
#include <mutex>
#include <type_traits>
#include <unordered_map>
#include "conv_epilogue.h"

using ds::f32x16;
typedef float f32x4 __attribute__((ext_vector_type(4)));   // native vector (HIP's float4 is a struct)
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) void *lds_ptr;

namespace {

constexpr int BK = 16;    // K-tile (floats)
constexpr int LDK = 20;   // padded LDS row stride for [row][k] tiles: 80 B, conflict-free b128 reads
using ds::kOOB;
using ds::make_srd;

struct ConvParams {
    ds_conv_desc d;
    const float *x;
    const float *w;
    float *z;
    const float *bias;
    const float *mask;
    float *stats;
    const float *pivot;   // per-column shift of the statistics (nullable)
    int M;          // N*OH*OW
    int taps;       // KH*KW
    int row_tiles;  // ceil(M/BM)
    unsigned x_bytes, w_bytes;   // extents covered by the two buffer descriptors
    int prio_mode;               // 1: staggered static wave priorities (see kernel)
    int col_tiles;               // > 0: 1-D XCD-aware launch (see TileId); 0: (row, column) = (blockIdx.x, blockIdx.y)
    int col_total;               // conv_bf16d_kernel: columns of the converted weight tensor (Cout rounded up to 32)
    ds_bn_bwd_on_load bnb;       // gemm_wide_kernel<.., BNB = true>: copy of *d.bnb (the descriptor's pointer is a host pointer)
    int pool_rpb, pool_bpi;      // gemm_wide_kernel<.., POOL = true>: image rows per 32-pixel block, blocks per image
    const float *scale, *shift;  // DS_EPI_BN_RELU (the <.., BNR = true> instantiations): Cout floats each
};

// Which tile does this workgroup own?  Two launch shapes:
//   * col_tiles == 0: 2-D grid, blockIdx.x = first row tile (persistent stride gridDim.x), blockIdx.y = column
//     tile; grid.x is a multiple of 8, so the column tiles of a row tile share an XCD.
//   * col_tiles > 0 (one workgroup per tile): 1-D grid, XCD-aware.  Workgroup id lands on XCD id % 8
//     (MI355X_MICROARCH.md, observed placement -- a different one only costs speed).  The row-major list of
//     (row tile, column tile) pairs is cut into 8 equal contiguous ranges, one per XCD, and consecutive ids of
//     ONE XCD walk its range: the workgroups that read the same A rows run on the same XCD back to back, so the
//     rows cross the fabric once per row tile instead of once per column tile (the 1x1 dgrad read its operand
//     4.6x, profiles/r01h_pmc_traffic.txt), and every XCD gets the same number of tiles whatever the tile
//     counts are (2 row tiles x 64 column tiles for an LSTM step included).  Up to 7 surplus workgroups find
//     row >= row_tiles and do nothing.
struct TileId {
    int row, col, stride;      // first row tile, column tile, row-tile stride of the persistent loop
};
// (bx, by) of a grid gx wide: the launch's own blockIdx / gridDim, or -- gemm_group_kernel -- a problem's share of a grouped launch
__device__ __forceinline__ TileId tile_id(const ConvParams &p, int bx, int by, int gx) {
    TileId t;
    if (p.col_tiles > 0) {
        const int id = bx;
        const int lin = (id & 7) * (gx >> 3) + (id >> 3);      // position in the row-major tile list
        t.row = lin / p.col_tiles;
        t.col = lin - t.row * p.col_tiles;
        t.stride = p.row_tiles;            // exactly one tile per workgroup
    } else {
        t.row = bx;
        t.col = by;
        t.stride = gx;
    }
    return t;
}
__device__ __forceinline__ TileId tile_id(const ConvParams &p) { return tile_id(p, (int)blockIdx.x, (int)blockIdx.y, (int)gridDim.x); }

template <bool VEC>
__device__ __forceinline__ f32x4 load4(__amdgpu_buffer_rsrc_t r, unsigned off, bool ok, int valid) {
    // off: byte offset of 4 consecutive floats; `valid` (<= 4) of them exist (scalar path only)
    if (VEC) {
        return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, ok ? off : kOOB, 0, 0));
    } else {
        f32x4 v;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            v[j] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, (ok && j < valid) ? off + 4 * j : kOOB, 0, 0));
        return v;
    }
}

// second launch-bound = waves per SIMD the register allocator must leave room for: the small tiles
// are the workhorses and measured fastest at 3-4 resident workgroups per CU
// BNR: the inference epilogue DS_EPI_BN_RELU, y = max(fma(acc, scale[col], shift[col]), 0) stored in place of z -- its own
// instantiation (forward, vector loads, MT = 1), so the training kernels' code is untouched
// floats of LDS one workgroup of conv_igemm_kernel<MT, NT, BNMAJOR, ..> stages its two K-tiles in
template <int MT, int NT, bool BNMAJOR>
constexpr int igemm_smem_floats() {
    return 2 * (4 * MT * 32) * LDK + 2 * (BNMAJOR ? BK * (NT * 32 + 4) : NT * 32 * LDK);
}

// One workgroup's share of a launch: the tiles `tid0` names, K-tiles of split `split` of `nsplits`.  The body of
// conv_igemm_kernel (its own blockIdx / gridDim) and of gemm_group_kernel (a problem's share of a grouped launch): the same
// loads, MFMAs and stores in the same order, so what a tile receives does not depend on which of the two launched it.
// `smem`: igemm_smem_floats<MT, NT, BNMAJOR>() floats, 16-byte aligned; wg_seq: the workgroup's number in dispatch order.
template <int MT, int NT, bool BNMAJOR, bool FOLD, bool VEC, bool BNR = false>
__device__ __forceinline__ void igemm_workgroup(const ConvParams &p, float *smem, const TileId tid0, const int split,
                                                const int nsplits, const int wg_seq) {
    constexpr int WM = 4;
    constexpr int BM = WM * MT * 32, BN = NT * 32;
    constexpr int AR = BM / 64;                       // float4 A loads per thread per K-tile
    constexpr int BR = (BN * 4 + 255) / 256;          // float4 B loads per thread per K-tile
    constexpr int LDB = BNMAJOR ? (BN + 4) : LDK;     // B tile: [k][n] (n-contiguous weights) or [n][k]
    constexpr int BSZ = BNMAJOR ? BK * LDB : BN * LDK;
    static_assert(igemm_smem_floats<MT, NT, BNMAJOR>() == 2 * BM * LDK + 2 * BSZ, "LDS size");
    float *As = smem;
    float *Bs = smem + 2 * BM * LDK;

    const ds_conv_desc &d = p.d;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wm = __builtin_amdgcn_readfirstlane(tid >> 6);   // provably wave-uniform
    const int li = lane & 31, lk = lane >> 5;
    const int n0 = tid0.col * BN;
    const int ohw = d.OH * d.OW;
    const int chunks = (d.Cin + BK - 1) / BK;
    // split-K (small-M GEMMs): split `split` owns K-tiles [kt0, kt1) and writes its own output slab
    const int KT_all = p.taps * chunks;
    const int kts = (KT_all + nsplits - 1) / nsplits;
    const int kt0 = split * kts;
    const int KT = (kt0 + kts < KT_all ? kt0 + kts : KT_all) - kt0;     // K-tiles of this split (may be <= 0)
    float *const zout = p.z + (int64_t)split * p.d.z_split_stride;
    const int flags = d.flags;
    const __amdgpu_buffer_rsrc_t srd_x = make_srd(p.x, p.x_bytes);
    const __amdgpu_buffer_rsrc_t srd_w = make_srd(p.w, p.w_bytes);

    // De-convoy the waves that share a SIMD.  With equal priority the matrix pipe is arbitrated fairly
    // among the 3-4 resident waves (one per co-resident workgroup), so they all finish their MFMA burst
    // together, all do their address/LDS/barrier phase together, and the pipe idles for that whole phase
    // (PMC: MFMA busy 72 %, idle share = non-MFMA phase / K-step).  Distinct static priorities make the
    // arbitration unfair: the phases stagger and one wave's non-MFMA work hides under another's MFMAs.
    // Co-resident workgroups are ~256 apart in dispatch order (id % 8 -> XCD, (id / 8) % 32 -> CU); a
    // different placement only costs speed.  s_setprio is scalar: the switch is wave-uniform.
    switch (p.prio_mode ? (wg_seq >> 8) & 3 : 0) {
        case 1: __builtin_amdgcn_s_setprio(1); break;
        case 2: __builtin_amdgcn_s_setprio(2); break;
        case 3: __builtin_amdgcn_s_setprio(3); break;
        default: break;
    }

    float csum[NT], csq[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) csum[j] = csq[j] = 0.f;

    const int arow = tid >> 2, ak4 = (tid & 3) * 4;

    // B-tile coordinates of this thread's loads are the same for every row tile and K-tile
    int b_n[BR], b_k[BR];
    unsigned b_off[BR];      // element offset inside one tap, without the K-tile base
    bool b_ok[BR];
#pragma unroll
    for (int i = 0; i < BR; ++i) {
        const int idx = tid + 256 * i;
        if (BNMAJOR) {       // n contiguous (forward): a float4 spans 4 output channels
            b_n[i] = n0 + (idx % (BN / 4)) * 4;
            b_k[i] = idx / (BN / 4);
            b_off[i] = (unsigned)b_k[i] * (unsigned)d.w_k_stride + (unsigned)b_n[i];
        } else {             // k contiguous (dgrad / transposed matmul): a float4 spans 4 reduction channels
            b_n[i] = n0 + (idx >> 2);
            b_k[i] = (idx & 3) * 4;
            b_off[i] = (unsigned)b_n[i] * (unsigned)d.w_n_stride + (unsigned)b_k[i];
        }
        b_ok[i] = idx < BN * 4 && b_n[i] < d.Cout;
    }

    // ---- loader state: the row tile and K-tile that the next load_tile() fetches ------------------
    int ih0[AR], iw0[AR];
    unsigned xb[AR];         // element offset of the image that row i belongs to
    int tap, c0, dh, dw;
    f32x4 ra[AR], rb[BR];
    f32x16 acc[MT][NT];

    auto setup_tile = [&](int tile) {      // point the loader at the first K-tile of row tile `tile`
        const int m0 = tile * BM;
#pragma unroll
        for (int i = 0; i < AR; ++i) {
            const int m = m0 + arow + 64 * i;
            const bool rv = m < p.M;
            const int mm = rv ? m : 0;
            const int n = mm / ohw;
            const int r = mm - n * ohw;
            const int oh = r / d.OW;
            const int ow = r - oh * d.OW;
            ih0[i] = rv ? oh * d.stride - d.pad_t : -(1 << 20);   // invalid rows fail the bounds test below
            iw0[i] = ow * d.stride - d.pad_l;
            xb[i] = (unsigned)n * (unsigned)(d.H * d.W) * (unsigned)d.ldx;
        }
        // K-tile order: channel chunk OUTER, tap INNER -- the KH*KW taps of one 16-channel chunk touch the
        // same (tile + halo) pixels' 64-byte segments, ~15 KB per workgroup, which stays in the XCD's L2
        // (tap-outer order streamed 9 x the whole tile through L2: measured 8x over-fetch on the 3x3 layers)
        const int chunk = kt0 / p.taps;
        tap = kt0 - chunk * p.taps;
        c0 = chunk * BK;
        dh = tap / d.KW;
        dw = tap - dh * d.KW;
    };

    {

        auto load_tile = [&]() {
            // ---- A: activations ----------------------------------------------------------------
            const int k = c0 + ak4;
#pragma unroll
            for (int i = 0; i < AR; ++i) {
                const int ih = ih0[i] + dh;
                const int iw = iw0[i] + dw;
                const int iwc = FOLD ? iw + k / d.fold_cin : iw;
                const bool ok = (unsigned)ih < (unsigned)d.H && (unsigned)iwc < (unsigned)d.W && k < d.Cin;
                const unsigned off = xb[i] + (unsigned)(ih * d.W + iw) * (unsigned)d.ldx + (unsigned)k;
                ra[i] = load4<VEC>(srd_x, off * 4u, ok, d.Cin - k);
            }
            // ---- B: weights, read in place from the HWIO tensor --------------------------------
            const int tap_eff = d.flip ? p.taps - 1 - tap : tap;
            const unsigned wt = (unsigned)tap_eff * (unsigned)d.w_tap_stride +
                                (unsigned)c0 * (BNMAJOR ? (unsigned)d.w_k_stride : 1u);
#pragma unroll
            for (int i = 0; i < BR; ++i) {
                const bool ok = b_ok[i] && c0 + b_k[i] < d.Cin;
                rb[i] = load4<VEC>(srd_w, (wt + b_off[i]) * 4u, ok, BNMAJOR ? d.Cout - b_n[i] : d.Cin - c0 - b_k[i]);
            }
            // ---- advance to the next K-tile: next tap of the same channel chunk, then the next chunk ----
            ++tap;
            if (++dw == d.KW) {
                dw = 0;
                if (++dh == d.KH) { dh = 0; tap = 0; c0 += BK; }
            }
        };

        auto store_tile = [&](int buf) {
            float *a_s = As + buf * BM * LDK;
            float *b_s = Bs + buf * BSZ;
#pragma unroll
            for (int i = 0; i < AR; ++i)
                *reinterpret_cast<f32x4 *>(a_s + (arow + 64 * i) * LDK + ak4) = ra[i];
#pragma unroll
            for (int i = 0; i < BR; ++i) {
                const int idx = tid + 256 * i;
                if (idx < BN * 4) {
                    if (BNMAJOR)
                        *reinterpret_cast<f32x4 *>(b_s + (idx / (BN / 4)) * LDB + (idx % (BN / 4)) * 4) = rb[i];
                    else
                        *reinterpret_cast<f32x4 *>(b_s + (idx >> 2) * LDK + (idx & 3) * 4) = rb[i];
                }
            }
        };

        auto compute = [&](int buf) {
            const float *a_s = As + buf * BM * LDK + (wm * MT * 32 + li) * LDK + lk * 8;
            float af[MT][8], bf[NT][8];
#pragma unroll
            for (int a = 0; a < MT; ++a) {
                const f32x4 lo = *reinterpret_cast<const f32x4 *>(a_s + a * 32 * LDK);
                const f32x4 hi = *reinterpret_cast<const f32x4 *>(a_s + a * 32 * LDK + 4);
                af[a][0] = lo.x; af[a][1] = lo.y; af[a][2] = lo.z; af[a][3] = lo.w;
                af[a][4] = hi.x; af[a][5] = hi.y; af[a][6] = hi.z; af[a][7] = hi.w;
            }
            if (BNMAJOR) {      // B staged [k][n]: lane (li, lk) needs B[k = lk*8+s][n = b*32+li]
                const float *b_s = Bs + buf * BSZ + (lk * 8) * LDB + li;
#pragma unroll
                for (int b = 0; b < NT; ++b)
#pragma unroll
                    for (int s = 0; s < 8; ++s) bf[b][s] = b_s[s * LDB + b * 32];
            } else {
                const float *b_s = Bs + buf * BSZ + li * LDK + lk * 8;
#pragma unroll
                for (int b = 0; b < NT; ++b) {
                    const f32x4 lo = *reinterpret_cast<const f32x4 *>(b_s + b * 32 * LDK);
                    const f32x4 hi = *reinterpret_cast<const f32x4 *>(b_s + b * 32 * LDK + 4);
                    bf[b][0] = lo.x; bf[b][1] = lo.y; bf[b][2] = lo.z; bf[b][3] = lo.w;
                    bf[b][4] = hi.x; bf[b][5] = hi.y; bf[b][6] = hi.z; bf[b][7] = hi.w;
                }
            }
#pragma unroll
            for (int s = 0; s < 8; ++s)
#pragma unroll
                for (int a = 0; a < MT; ++a)
#pragma unroll
                    for (int b = 0; b < NT; ++b)
                        acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[a][s], bf[b][s], acc[a][b], 0, 0, 0);
        };

    // One continuous software pipeline over (row tile, K-tile): while the MFMAs of K-tile kt run, the
    // loads of kt+1 are in flight; on the LAST K-tile of a row tile the loads already belong to the
    // first K-tile of the NEXT row tile, so the pipeline never drains between tiles and the epilogue
    // of tile t starts with tile t+1's operands already staged in LDS.
    int par = 0;                                   // LDS buffer holding the K-tile about to be computed
    if (tid0.row < p.row_tiles) {
        setup_tile(tid0.row);
        load_tile();
        store_tile(0);
    }
    __syncthreads();
    for (int tile = tid0.row; tile < p.row_tiles; tile += tid0.stride) {
        const int m0 = tile * BM;
        const bool has_next = tile + tid0.stride < p.row_tiles;
#pragma unroll
        for (int a = 0; a < MT; ++a)
#pragma unroll
            for (int b = 0; b < NT; ++b)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;
        for (int kt = 0; kt < KT; ++kt) {
            const bool last = kt + 1 == KT;
            if (last && has_next) setup_tile(tile + tid0.stride);
            const bool fetch = !last || has_next;
            if (fetch) load_tile();
            compute(par);
            if (fetch) store_tile(par ^ 1);
            __syncthreads();
            par ^= 1;
        }

        // ---- epilogue (conv_epilogue.h): bias / accumulate / mask / relu, store, BatchNorm column statistics -------
        ds::tile_store<MT, NT, BNR>(p.d, p.M, zout, p.bias, p.mask, p.pivot, p.scale, p.shift, [&](int a, int b) -> const f32x16 & { return acc[a][b]; },
                                    m0 + wm * MT * 32 + 4 * lk, n0 + li, csum, csq);
    }
    }

    if (flags & DS_EPI_STATS)      // (red = the operand tiles: every wave passed the last K-loop barrier)
        ds::tile_stats_combine<NT>(smem, csum, csq, n0, d.Cout, tid0.row < p.row_tiles, p.stats, tid0.stride, tid0.row);
}

template <int MT, int NT, bool BNMAJOR, bool FOLD, bool VEC, bool BNR = false>
__global__ __launch_bounds__(256, (MT == 1 && NT == 1) ? 4 : (MT == 1 && NT == 2) ? 3 : 1) void conv_igemm_kernel(
    const ConvParams p) {
    __shared__ __attribute__((aligned(16))) float smem[igemm_smem_floats<MT, NT, BNMAJOR>()];
    igemm_workgroup<MT, NT, BNMAJOR, FOLD, VEC, BNR>(
        p, smem, tile_id(p), (int)blockIdx.z, (int)gridDim.z,
        (int)(blockIdx.x + blockIdx.y * gridDim.x + blockIdx.z * gridDim.x * gridDim.y));
}

// ---- grouped launch of up to four independent batch x features GEMMs (ds_gemm_group) ---------------------------------
// The joint head's GEMMs are a row tile or two each: a launch of theirs fills a fraction of the chip and costs a dependent-launch
// boundary.  Problems that do not depend on each other (W_fc's image and text halves) share ONE launch: the grid is the
// concatenation of the problems' grids, every workgroup looks its problem up once -- scalar code, before the K loop -- and then
// runs igemm_workgroup<1, 1, ..> on it exactly as that problem's own ds_conv_igemm launch would.
constexpr int kGemmGroupMax = 4;
struct GemmGroupParams {
    ConvParams p[kGemmGroupMax];
    int wg_end[kGemmGroupMax];       // first workgroup past problem i
    int gx[kGemmGroupMax], gy[kGemmGroupMax], splits[kGemmGroupMax];      // the grid ds_conv_igemm launches for problem i
    int variant[kGemmGroupMax];      // bit 0: n-contiguous weights (BNMAJOR), bit 1: 16-byte loads (VEC)
    int count;
};

__global__ __launch_bounds__(256, 4) void gemm_group_kernel(const GemmGroupParams g) {
    constexpr int kSmem = igemm_smem_floats<1, 1, true>() > igemm_smem_floats<1, 1, false>() ? igemm_smem_floats<1, 1, true>()
                                                                                              : igemm_smem_floats<1, 1, false>();
    __shared__ __attribute__((aligned(16))) float smem[kSmem];
    const int id = (int)blockIdx.x;
    int q = 0;
    while (q + 1 < g.count && id >= g.wg_end[q]) ++q;
    const int local = id - (q ? g.wg_end[q - 1] : 0);
    const int gx = g.gx[q], gxy = gx * g.gy[q];
    const int split = local / gxy;
    const int by = (local - split * gxy) / gx;
    const int bx = local - split * gxy - by * gx;
    const ConvParams &p = g.p[q];
    const TileId t = tile_id(p, bx, by, gx);
    switch (g.variant[q]) {
        case 0: igemm_workgroup<1, 1, false, false, false>(p, smem, t, split, g.splits[q], local); break;
        case 1: igemm_workgroup<1, 1, true, false, false>(p, smem, t, split, g.splits[q], local); break;
        case 2: igemm_workgroup<1, 1, false, false, true>(p, smem, t, split, g.splits[q], local); break;
        default: igemm_workgroup<1, 1, true, false, true>(p, smem, t, split, g.splits[q], local); break;
    }
}

// ================================================================================================
// LDS-DMA variant (gfx950): K-tile 32, operands go global -> LDS with buffer_load_dwordx4 ... lds.
//
// Same implicit GEMM, same epilogue, different staging.  conv_igemm_kernel's loop moves every operand through
// VGPRs (buffer_load -> s_waitcnt -> ds_write_b128): 12 staging registers per thread, three 13-cycle
// LDS stores per K-tile and a vmcnt(0) in the middle of every K-step.  Here each lane's 16 bytes land
// directly in LDS (a wave-instruction fills 1 KiB at M0 + lane*16; out-of-range lanes write zeros --
// probed in scripts/microbench/glds_test.hip), so there are no staging registers and no LDS stores, and the
// freed registers pay for a 32-deep K-tile: half as many barriers and fragment-read restarts per MFMA.
// Rows are 128 bytes and unpadded (the DMA destination is lane-linear), so the bank-conflict-free layout
// is an XOR swizzle applied on the SOURCE side: LDS slot (row, pc) holds the row's logical 16-byte chunk
// pc ^ ((row >> 1) & 7), and fragment reads apply the same involution (cdna_hip_programming.md rule 21).
// With ds_read_b128's lane groups {0-3,12-15,20-27} / {4-11,16-19,28-31} the eight rows of equal parity
// in a group map to eight different chunk columns: conflict-free.
// Per K-step: read all fragments of the current tile, issue the DMAs of the next tile, run the MFMAs,
// __syncthreads() (hipcc puts the vmcnt(0) for the DMAs there).
// ================================================================================================
constexpr int GK = 32;            // K-tile (floats)
constexpr int GCH = GK / 4;       // 16-byte chunks per row

template <int NT, bool BNMAJOR, bool BNR = false>      // BNR: DS_EPI_BN_RELU (see conv_igemm_kernel)
__global__ __launch_bounds__(256, NT == 1 ? 4 : (NT == 2 ? 3 : 2)) void conv_glds_kernel(const ConvParams p) {
    constexpr int BM = 128, BN = NT * 32;
    constexpr int ASZ = BM * GK, BSZ = BN * GK;       // floats per buffer
    constexpr int AJ = BM * GCH / 256;                // A DMA instructions per thread per K-tile (4)
    constexpr int BJ = BN * GCH / 256;                // B DMA instructions per thread per K-tile (NT)
    __shared__ __attribute__((aligned(128))) float smem[2 * ASZ + 2 * BSZ];
    float *As = smem;
    float *Bs = smem + 2 * ASZ;

    const ds_conv_desc &d = p.d;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wm = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 31, lk = lane >> 5;
    const TileId tid0 = tile_id(p);
    const int n0 = tid0.col * BN;
    const int ohw = d.OH * d.OW;
    const int chunks = (d.Cin + GK - 1) / GK;
    const int KT_all = p.taps * chunks;
    const int kts = (KT_all + (int)gridDim.z - 1) / (int)gridDim.z;
    const int kt0 = (int)blockIdx.z * kts;
    const int KT = (kt0 + kts < KT_all ? kt0 + kts : KT_all) - kt0;
    float *const zout = p.z + (int64_t)blockIdx.z * p.d.z_split_stride;
    const int flags = d.flags;
    const __amdgpu_buffer_rsrc_t srd_x = make_srd(p.x, p.x_bytes);
    const __amdgpu_buffer_rsrc_t srd_w = make_srd(p.w, p.w_bytes);

    float csum[NT], csq[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) csum[j] = csq[j] = 0.f;

    // ---- DMA slot of this thread: slot = j*256 + tid -> (row j*32 + tid/8, physical chunk tid%8) ------
    const int srow = tid >> 3;                                   // + 32*j
    const int slc4 = ((tid & 7) ^ ((tid >> 4) & 7)) * 4;         // logical k offset of the chunk it fetches
    // B, k-contiguous weights: same slot shape, rows are output channels
    // B, n-contiguous weights: tile is [k][n], slot -> (k = slot / (BN/4), n4 = slot % (BN/4)), no swizzle
    int b_row[BJ], b_col[BJ];
    bool b_ok[BJ];
#pragma unroll
    for (int i = 0; i < BJ; ++i) {
        const int slot = i * 256 + tid;
        if (BNMAJOR) {
            b_row[i] = slot / (BN / 4);                          // k inside the tile
            b_col[i] = n0 + (slot % (BN / 4)) * 4;               // first of 4 output channels
            b_ok[i] = b_col[i] < d.Cout;
        } else {
            b_row[i] = n0 + i * 32 + srow;                       // output channel
            b_col[i] = slc4;                                     // k inside the tile
            b_ok[i] = b_row[i] < d.Cout;
        }
    }

    int ih0[AJ], iw0[AJ];
    unsigned xb[AJ];
    int tap, c0, dh, dw;
    f32x16 acc[NT];

    auto setup_tile = [&](int tile) {
        const int m0 = tile * BM;
#pragma unroll
        for (int j = 0; j < AJ; ++j) {
            const int m = m0 + j * 32 + srow;
            const bool rv = m < p.M;
            const int mm = rv ? m : 0;
            const int n = mm / ohw;
            const int r = mm - n * ohw;
            const int oh = r / d.OW;
            const int ow = r - oh * d.OW;
            ih0[j] = rv ? oh * d.stride - d.pad_t : -(1 << 20);
            iw0[j] = ow * d.stride - d.pad_l;
            xb[j] = (unsigned)n * (unsigned)(d.H * d.W) * (unsigned)d.ldx;
        }
        const int chunk = kt0 / p.taps;                          // channel chunk outer, tap inner
        tap = kt0 - chunk * p.taps;
        c0 = chunk * GK;
        dh = tap / d.KW;
        dw = tap - dh * d.KW;
    };

    auto issue_tile = [&](int buf) {       // DMA the K-tile the loader points at into buffer `buf`, then advance
        float *a_s = As + buf * ASZ + wm * 256;                  // this wave's 1 KiB window of pass j = 0
        const int ka = c0 + slc4;
#pragma unroll
        for (int j = 0; j < AJ; ++j) {
            const int ih = ih0[j] + dh;
            const int iw = iw0[j] + dw;
            const bool ok = (unsigned)ih < (unsigned)d.H && (unsigned)iw < (unsigned)d.W && ka < d.Cin;
            const unsigned off = xb[j] + (unsigned)(ih * d.W + iw) * (unsigned)d.ldx + (unsigned)ka;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(srd_x, (lds_ptr)(a_s + j * 1024), 16, ok ? off * 4u : kOOB, 0, 0, 0);
        }
        const int tap_eff = d.flip ? p.taps - 1 - tap : tap;
        const unsigned wt = (unsigned)tap_eff * (unsigned)d.w_tap_stride;
        float *b_s = Bs + buf * BSZ + wm * 256;
#pragma unroll
        for (int i = 0; i < BJ; ++i) {
            bool ok;
            unsigned off;
            if (BNMAJOR) {
                const int k = c0 + b_row[i];
                ok = b_ok[i] && k < d.Cin;
                off = wt + (unsigned)k * (unsigned)d.w_k_stride + (unsigned)b_col[i];
            } else {
                const int k = c0 + b_col[i];
                ok = b_ok[i] && k < d.Cin;
                off = wt + (unsigned)b_row[i] * (unsigned)d.w_n_stride + (unsigned)k;
            }
            __builtin_amdgcn_raw_ptr_buffer_load_lds(srd_w, (lds_ptr)(b_s + i * 1024), 16, ok ? off * 4u : kOOB, 0, 0, 0);
        }
        ++tap;
        if (++dw == d.KW) {
            dw = 0;
            if (++dh == d.KH) { dh = 0; tap = 0; c0 += GK; }
        }
    };

    // fragment addresses: lane (li, lk) owns k = lk*16 .. lk*16+15 of its row = logical chunks lk*4 .. lk*4+3
    const int arow = wm * 32 + li;
    const int asw = (arow >> 1) & 7;
    int a_off[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) a_off[c] = arow * GK + (((lk * 4 + c) ^ asw) * 4);
    int b_offk[NT][4];
    if (!BNMAJOR) {
#pragma unroll
        for (int b = 0; b < NT; ++b) {
            const int brow = b * 32 + li;
#pragma unroll
            for (int c = 0; c < 4; ++c) b_offk[b][c] = brow * GK + (((lk * 4 + c) ^ ((brow >> 1) & 7)) * 4);
        }
    }

    float af[16], bf[NT][16];
    auto read_frags = [&](int buf) {
        const float *a_s = As + buf * ASZ;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const f32x4 v = *reinterpret_cast<const f32x4 *>(a_s + a_off[c]);
            af[4 * c + 0] = v.x; af[4 * c + 1] = v.y; af[4 * c + 2] = v.z; af[4 * c + 3] = v.w;
        }
        const float *b_s = Bs + buf * BSZ;
        if (BNMAJOR) {
            const float *bp = b_s + (lk * 16) * BN + li;
#pragma unroll
            for (int b = 0; b < NT; ++b)
#pragma unroll
                for (int s = 0; s < 16; ++s) bf[b][s] = bp[s * BN + b * 32];
        } else {
#pragma unroll
            for (int b = 0; b < NT; ++b)
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const f32x4 v = *reinterpret_cast<const f32x4 *>(b_s + b_offk[b][c]);
                    bf[b][4 * c + 0] = v.x; bf[b][4 * c + 1] = v.y; bf[b][4 * c + 2] = v.z; bf[b][4 * c + 3] = v.w;
                }
        }
    };
    auto mfmas = [&]() {
#pragma unroll
        for (int s = 0; s < 16; ++s)
#pragma unroll
            for (int b = 0; b < NT; ++b) acc[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[s], bf[b][s], acc[b], 0, 0, 0);
    };

    int par = 0;
    if (tid0.row < p.row_tiles) {
        setup_tile(tid0.row);
        issue_tile(0);
    }
    __syncthreads();
    for (int tile = tid0.row; tile < p.row_tiles; tile += tid0.stride) {
        const int m0 = tile * BM;
        const bool has_next = tile + tid0.stride < p.row_tiles;
#pragma unroll
        for (int b = 0; b < NT; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[b][r] = 0.f;
        for (int kt = 0; kt < KT; ++kt) {
            const bool last = kt + 1 == KT;
            read_frags(par);
            if (last && has_next) setup_tile(tile + tid0.stride);
            if (!last || has_next) issue_tile(par ^ 1);
            __builtin_amdgcn_sched_barrier(0);     // DMAs are issued before the MFMAs ...
            mfmas();
            __builtin_amdgcn_sched_barrier(0);     // ... and the MFMAs stay above the barrier's vmcnt(0)
            __syncthreads();
            par ^= 1;
        }

        // ---- epilogue (conv_epilogue.h): bias / accumulate / mask / relu, store, BatchNorm column statistics -------
        ds::tile_store<1, NT, BNR>(p.d, p.M, zout, p.bias, p.mask, p.pivot, p.scale, p.shift, [&](int, int b) -> const f32x16 & { return acc[b]; },
                                   m0 + wm * 32 + 4 * lk, n0 + li, csum, csq);
    }

    if (flags & DS_EPI_STATS)      // (red = the operand tiles: every wave passed the last K-loop barrier and no DMA is in flight)
        ds::tile_stats_combine<NT>(smem, csum, csq, n0, d.Cout, tid0.row < p.row_tiles, p.stats, tid0.stride, tid0.row);
}


// ================================================================================================
// bf16-multiply variant (ds_conv_desc.dtype == DS_DTYPE_BF16): v_mfma_f32_32x32x16_bf16, fp32 accumulate.
//
// BASELINE configs[4] groundwork.  Storage is unchanged -- activations, weights (masters), BatchNorm statistics
// and z stay fp32 in HBM -- only the multiply runs on the bf16 matrix pipe (16x the fp32 MFMA rate): operands are
// rounded to bf16 (round-to-nearest-even, v_cvt_pk_bf16_f32) on their way from the staging registers into LDS.
// Same implicit GEMM, same SRD loads with hardware zero fill, same epilogue (bias / accumulate / mask / relu /
// BatchNorm column statistics about the pivot, all in fp32 from the fp32 accumulators).
//   * K-tile 32 channels of one tap; both tiles live in LDS as [row][k] bf16 rows of 64 B padded to 80 B
//     (20-bank row stride: the sixteen rows of a ds_read_b128 lane group cover the 64 banks exactly once);
//   * A fragment of the 32x32x16 MFMA = lane (i, kh) holds A[i][8 kh .. 8 kh + 7] = one ds_read_b128; the B tile is
//     stored [n][k] for both weight layouts (n-contiguous HWIO weights are transposed on the LDS store by packing
//     the (k, k+1) pair of each of the four columns of a float4 into one dword);
//   * at 16x the matrix rate the loop is bound by operand staging, so tiles are 128 x 128 (NT = 4) wherever Cout
//     allows: 32 KB of fp32 operands staged per 1 MFLOP.
// Numerics: products of bf16-rounded operands, exact fp32 accumulation in k order; against the fp32 path the
// relative error is ~2^-9 per operand (documented tolerance of the bf16 parity tests: 1e-2 of max |ref|).
// ================================================================================================
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

constexpr int HK = 32;       // K-tile (channels)
constexpr int HLD = 40;      // LDS row stride in bf16 elements (80 B)

template <int NT, bool BNMAJOR, bool FOLD>
__global__ __launch_bounds__(256, NT <= 2 ? 3 : 2) void conv_bf16_kernel(const ConvParams p) {
    constexpr int BM = 128, BN = NT * 32;
    constexpr int AJ = 4;                                                // float4 A loads per thread per K-tile
    constexpr int BP = BNMAJOR ? (4 * BN + 255) / 256 : 0;               // (k, k+1) x float4(n) pairs per thread
    constexpr int BJ = BNMAJOR ? 0 : BN / 32;                            // float4(k) loads per thread
    constexpr int NB = BNMAJOR ? 2 * BP : BJ;
    __shared__ __attribute__((aligned(16))) __bf16 smem[2 * BM * HLD + 2 * BN * HLD];
    __bf16 *As = smem;
    __bf16 *Bs = smem + 2 * BM * HLD;

    const ds_conv_desc &d = p.d;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wm = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 31, kh = lane >> 5;
    const TileId tid0 = tile_id(p);
    const int n0 = tid0.col * BN;
    const int ohw = d.OH * d.OW;
    const int chunks = (d.Cin + HK - 1) / HK;
    const int KT = p.taps * chunks;
    float *const zout = p.z;
    const int flags = d.flags;
    const __amdgpu_buffer_rsrc_t srd_x = make_srd(p.x, p.x_bytes);
    const __amdgpu_buffer_rsrc_t srd_w = make_srd(p.w, p.w_bytes);

    float csum[NT], csq[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) csum[j] = csq[j] = 0.f;

    const int srow = tid >> 3, c4 = (tid & 7) * 4;        // A slot: rows srow + 32 j, channels c4 .. c4 + 3 of the K-tile
    int ih0[AJ], iw0[AJ];
    unsigned xb[AJ];
    int tap, c0, dh, dw;
    f32x4 ra[AJ], rb[NB > 0 ? NB : 1];
    f32x16 acc[NT];

    auto setup_tile = [&](int tile) {
        const int m0 = tile * BM;
#pragma unroll
        for (int j = 0; j < AJ; ++j) {
            const int m = m0 + srow + 32 * j;
            const bool rv = m < p.M;
            const int mm = rv ? m : 0;
            const int n = mm / ohw;
            const int r = mm - n * ohw;
            const int oh = r / d.OW;
            const int ow = r - oh * d.OW;
            ih0[j] = rv ? oh * d.stride - d.pad_t : -(1 << 20);
            iw0[j] = ow * d.stride - d.pad_l;
            xb[j] = (unsigned)n * (unsigned)(d.H * d.W) * (unsigned)d.ldx;
        }
        tap = 0; c0 = 0; dh = 0; dw = 0;                  // channel chunk outer, tap inner (as the fp32 kernels)
    };

    auto load_tile = [&]() {
        const int k = c0 + c4;
#pragma unroll
        for (int j = 0; j < AJ; ++j) {
            const int ih = ih0[j] + dh;
            const int iw = iw0[j] + dw;
            const int iwc = FOLD ? iw + k / d.fold_cin : iw;
            const bool ok = (unsigned)ih < (unsigned)d.H && (unsigned)iwc < (unsigned)d.W && k < d.Cin;
            const unsigned off = xb[j] + (unsigned)(ih * d.W + iw) * (unsigned)d.ldx + (unsigned)k;
            ra[j] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(srd_x, ok ? off * 4u : kOOB, 0, 0));
        }
        const int tap_eff = d.flip ? p.taps - 1 - tap : tap;
        const unsigned wt = (unsigned)tap_eff * (unsigned)d.w_tap_stride;
        if (BNMAJOR) {
#pragma unroll
            for (int i = 0; i < BP; ++i) {
                const int pi = tid + 256 * i;
                const int kp = pi / (BN / 4), n4 = pi - kp * (BN / 4);
                const int kk = c0 + 2 * kp, nn = n0 + 4 * n4;
                const bool okn = pi < 4 * BN && nn < d.Cout;
                const unsigned off = wt + (unsigned)kk * (unsigned)d.w_k_stride + (unsigned)nn;
                rb[2 * i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(srd_w, (okn && kk < d.Cin) ? off * 4u : kOOB, 0, 0));
                rb[2 * i + 1] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(
                                                       srd_w, (okn && kk + 1 < d.Cin) ? (off + (unsigned)d.w_k_stride) * 4u : kOOB, 0, 0));
            }
        } else {
#pragma unroll
            for (int i = 0; i < BJ; ++i) {
                const int nn = n0 + srow + 32 * i;
                const bool ok = nn < d.Cout && k < d.Cin;
                const unsigned off = wt + (unsigned)nn * (unsigned)d.w_n_stride + (unsigned)k;
                rb[i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(srd_w, ok ? off * 4u : kOOB, 0, 0));
            }
        }
        ++tap;
        if (++dw == d.KW) {
            dw = 0;
            if (++dh == d.KH) { dh = 0; tap = 0; c0 += HK; }
        }
    };

    auto store_tile = [&](int buf) {
        __bf16 *a_s = As + buf * BM * HLD;
        __bf16 *b_s = Bs + buf * BN * HLD;
#pragma unroll
        for (int j = 0; j < AJ; ++j)
            *reinterpret_cast<bf16x4 *>(a_s + (srow + 32 * j) * HLD + c4) = __builtin_convertvector(ra[j], bf16x4);
        if (BNMAJOR) {
#pragma unroll
            for (int i = 0; i < BP; ++i) {
                const int pi = tid + 256 * i;
                const int kp = pi / (BN / 4), n4 = pi - kp * (BN / 4);
                if (pi < 4 * BN) {
#pragma unroll
                    for (int jj = 0; jj < 4; ++jj) {
                        const f32x2 pr = {rb[2 * i][jj], rb[2 * i + 1][jj]};
                        *reinterpret_cast<bf16x2 *>(b_s + (4 * n4 + jj) * HLD + 2 * kp) = __builtin_convertvector(pr, bf16x2);
                    }
                }
            }
        } else {
#pragma unroll
            for (int i = 0; i < BJ; ++i)
                *reinterpret_cast<bf16x4 *>(b_s + (srow + 32 * i) * HLD + c4) = __builtin_convertvector(rb[i], bf16x4);
        }
    };

    auto compute = [&](int buf) {
        const __bf16 *a_s = As + buf * BM * HLD + (wm * 32 + li) * HLD + kh * 8;
        const __bf16 *b_s = Bs + buf * BN * HLD + li * HLD + kh * 8;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const bf16x8 a = *reinterpret_cast<const bf16x8 *>(a_s + ks * 16);
#pragma unroll
            for (int b = 0; b < NT; ++b) {
                const bf16x8 w = *reinterpret_cast<const bf16x8 *>(b_s + b * 32 * HLD + ks * 16);
                acc[b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, w, acc[b], 0, 0, 0);
            }
        }
    };

    int par = 0;
    if (tid0.row < p.row_tiles) {
        setup_tile(tid0.row);
        load_tile();
        store_tile(0);
    }
    __syncthreads();
    for (int tile = tid0.row; tile < p.row_tiles; tile += tid0.stride) {
        const int m0 = tile * BM;
        const bool has_next = tile + tid0.stride < p.row_tiles;
#pragma unroll
        for (int b = 0; b < NT; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[b][r] = 0.f;
        for (int kt = 0; kt < KT; ++kt) {
            const bool last = kt + 1 == KT;
            if (last && has_next) setup_tile(tile + tid0.stride);
            const bool fetch = !last || has_next;
            if (fetch) load_tile();
            compute(par);
            if (fetch) store_tile(par ^ 1);
            __syncthreads();
            par ^= 1;
        }
        // The tile epilogue (ds::tile_store, ds::tile_stats_combine) in place: on the shared functions this kernel gains occupancy,
        // and a persistent launch sizes its grid and partial count by it (profiles/conv_epilogue_notes.md).
#pragma unroll
        for (int b = 0; b < NT; ++b) {
            const int col = n0 + b * 32 + li;
            const bool colok = col < d.Cout;
            const float bv = ((flags & DS_EPI_BIAS) && colok) ? p.bias[col] : 0.f;
            const float pv = (p.pivot && colok) ? p.pivot[col] : 0.f;
            float s = 0.f, q = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = m0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh;
                if (row < p.M && colok) {
                    float v = acc[b][r] + bv;
                    const int64_t off = (int64_t)row * d.ldz + col;
                    if (flags & DS_EPI_ACCUM) v += zout[off];
                    if (flags & DS_EPI_MASK) v = p.mask[(int64_t)row * d.ldmask + col] > 0.f ? v : 0.f;
                    if (flags & DS_EPI_RELU) v = fmaxf(v, 0.f);
                    zout[off] = v;
                    const float u = v - pv;
                    s += u;
                    q += u * u;
                }
            }
            csum[b] += s;
            csq[b] += q;
        }
    }

    if (flags & DS_EPI_STATS) {
        float *red = reinterpret_cast<float *>(smem);   // [4][BN][2] floats; every wave passed the last K-loop barrier
        __syncthreads();
#pragma unroll
        for (int b = 0; b < NT; ++b) {
            const float s = csum[b] + __shfl_xor(csum[b], 32);
            const float q = csq[b] + __shfl_xor(csq[b], 32);
            if (kh == 0) {
                const int c = b * 32 + li;
                red[(wm * BN + c) * 2 + 0] = s;
                red[(wm * BN + c) * 2 + 1] = q;
            }
        }
        __syncthreads();
        if (tid < BN && n0 + tid < d.Cout && tid0.row < p.row_tiles) {
            float s = 0.f, q = 0.f;
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                s += red[(w * BN + tid) * 2 + 0];
                q += red[(w * BN + tid) * 2 + 1];
            }
            p.stats[(int64_t)(n0 + tid) * tid0.stride + tid0.row] = s;
            p.stats[((int64_t)d.Cout + n0 + tid) * tid0.stride + tid0.row] = q;
        }
    }
}


// ================================================================================================
// Wide-tile 1x1 / GEMM variant: one wave per 32 rows x (NB * 32) columns, A operand register-direct.
//
// The 1x1 layers (Branch_0/1/2 Conv2d_0a_1x1 fused, Branch_3 Conv2d_0b_1x1, Conv2d_2b_1x1 and their dgrads) have no
// spatial footprint: row m of the A operand IS pixel m.  So the structure that made the Winograd kernel fast applies
// without the transform: lane (i, kh) of the 32x32x2 MFMA loads channels 4 kh .. 4 kh + 3 of row i as one float4 and
// that IS its A fragment -- no LDS round trip for A, no barrier on its account -- and every A fragment is used for
// NB * 4 MFMAs (NB up to 8: 256 columns, 128 accumulator registers) instead of 2 * 4 in the 128 x 64 LDS tile.  The B
// operand (a [16 k][NB*32] slice of the weights per K step, read in place from the HWIO tensor) goes global -> LDS by
// LDS-DMA, double buffered, shared by the workgroup's four waves (four 32-row groups); its fragments are read
// position by position in the shadow of the MFMAs, and the loads / DMAs of the next K step are issued BETWEEN the
// MFMA groups (conv_wino.hip: a burst of row-scattered loads stalls the in-order wave behind the texture path).
// Epilogue: stores (DS_EPI_ACCUM: z += result) + BatchNorm column statistics about the pivot (DS_EPI_STATS).
// ================================================================================================
// BNB (dgrad of a 1x1 conv + BatchNorm + ReLU layer, ds_conv_desc.bnb): x holds the layer's z and the A fragment becomes
// dz = bn_bwd_dz(z, dy, ...) as it is loaded -- a second float4 (dy, from up to three channel ranges whose boundaries are
// multiples of the 16-channel K step, so a step's range is wave-uniform) and five per-channel values from LDS per A
// float4, ~8 VALU per element against NB MFMAs: the layer's ds_bn_bwd_apply pass (12 B per element) disappears.
// Both A loads of the next K step are issued back to back: a row's 16 channels are ONE 64-byte sector, and with the second
// load a column block (8 MFMAs x the resident waves) behind the first the sector had left the 32 KB L1 again -- 19.8 M
// L1 -> L2 read requests per launch on the 28 x 28, 256 -> 288 layer against 9.6 M sectors of A (rocprofv3 TCP_TCC_READ_REQ,
// profiles/r05_notes.md).  Fifteen 1x1 shapes: dgrad with accumulate + sums 2399 -> 2334 us, step 14.51 -> 14.39 ms.
#ifndef DS_WIDE_A_B2B
#define DS_WIDE_A_B2B 1
#endif
// POOL (ds_conv_desc.pool_argmax: an Inception block's Branch_3, MaxPool 3x3/1 SAME -> Conv2d_0b_1x1, as ONE launch): the A
// fragment of pixel (h, w) becomes the maximum of x over its 3x3 neighbourhood as it is loaded.  A wave's 32-row block holds
// WHOLE image rows (28 of 32 lanes on the 28 / 14 / 7-wide maps), so that a pixel's left and right neighbours are the
// neighbouring lanes: lane (pixel, kh) takes its own column -- rows h-1, h, h+1, the same 2 x 4 channels -- forms the column
// maximum and the first row that holds it, gets its neighbours' column maxima by two DPP wave shifts and keeps the
// row-major-first winner (kh * 3 + kw: what maxpool3_fwd_rolling records).  The three rows come from an LDS tile of the
// workgroup's centre rows (its four blocks are consecutive row groups), which the waves fill with one 64-byte sector per lane
// quad; only the row above wave 0's block and the one below wave 3's are read from memory a second time.  The fragment
// layout took all three rows from memory, four rows per lane quad: 454 L1 tag lookups per wave and K step, 1.96 cycles
// each, was the whole launch time on the 28 x 28 maps (profiles/pool_on_load_notes.md).
// With norm_rstd / norm_shift the maximum is taken over the raw z and relu(max * rstd + shift) applied once (rstd > 0), as
// ds_maxpool_bn_relu_fwd does.  The winners' bytes are the only thing besides z that is written: the pooled tensor
// (4 B per element out of the pool kernel and 4 B back into this one) never exists.
template <bool BNR>
struct WideEpi : ds::WaveRowOpt { static constexpr bool bnr = BNR, mask_rstd = true; };

template <int NB, bool BNMAJOR, bool BNB = false, bool POOL = false, bool BNR = false>      // BNR: DS_EPI_BN_RELU (see conv_igemm_kernel)
__global__ __launch_bounds__(256, NB <= 4 ? 3 : 2) void gemm_wide_kernel(const ConvParams p) {
    constexpr int BN = NB * 32, WK = 16;                       // K step: 16 channels = two float4 per lane
    constexpr int DJ = (WK * BN / 4 + 255) / 256;              // 16-byte DMA slots per thread per K step: ceil(NB / 2)
    constexpr int BSZ = DJ * 1024;                             // floats per B buffer (odd NB: the last DMA is half used)
    constexpr int BST = 2;                                     // B buffers
    constexpr int PT = 2048;                                   // POOL: floats per centre-row tile (128 pixels x 16 channels)
    __shared__ __attribute__((aligned(128))) float smem[BST * BSZ + 256 + (POOL ? 2 * PT : 0)];
    // BatchNorm + ReLU on load (ds_conv_desc.norm_rstd / norm_shift): rstd and shift of all Cin reduction channels;
    // BNB: rstd, shift, mean, coef[0], coef[1]
    __shared__ __attribute__((aligned(16))) float nrm[BNB ? 5 : 2][1024 + WK];
    const ds_conv_desc &d = p.d;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 31, kh = lane >> 5;
    const TileId t0 = tile_id(p);
    const int n0 = t0.col * BN;
    const bool item = t0.row < p.row_tiles;
    const __amdgpu_buffer_rsrc_t srd_x = make_srd(p.x, p.x_bytes);
    const __amdgpu_buffer_rsrc_t srd_w = make_srd(p.w, p.w_bytes);
    const int K = d.Cin;
    // this wave's 32-row block: rows mrow0 ... of the output, the first Mw - mrow0 of them real
    int mrow0 = t0.row * 128 + wave * 32, Mw = p.M;
    bool hasU = false, hasD = false, hasL = false, hasR = false;      // POOL: which neighbours of the lane's pixel exist
    int prow = 0;                                                     // POOL: bytes between image rows of x
    // POOL: where the pixel above / below comes from.  The workgroup's four blocks are consecutive row groups, so it is a
    // pixel of this wave's block, of the neighbouring wave's block -- both in the centre-row tile in LDS (pu / pd: its pixel
    // slot, the lane's own where there is no neighbour or it comes from memory) -- or, for the first row of wave 0 and the
    // last row of wave 3, a halo row read from memory (upM / dnM)
    bool upM = false, dnM = false;
    int pu = 0, pd = 0;
    if constexpr (POOL) {
        const int blk = t0.row * 4 + wave;                           // (uniform)
        const int n = blk / p.pool_bpi, rb = blk - n * p.pool_bpi;
        const int r0 = rb * p.pool_rpb;
        const int rows = (d.H - r0) < p.pool_rpb ? (d.H - r0) : p.pool_rpb;
        const int cnt = (item && n < d.N) ? rows * d.W : 0;
        mrow0 = (n * d.H + r0) * d.W;
        Mw = mrow0 + cnt;
        const int dr = li / d.W, ow = li - dr * d.W, oh = r0 + dr;
        const bool ok = li < cnt;
        hasU = ok && oh > 0;
        hasD = ok && oh + 1 < d.H;
        hasL = ok && ow > 0;
        hasR = ok && ow + 1 < d.W;
        prow = d.W * d.ldx * 4;
        const bool top = dr == 0, bot = dr + 1 == rows;              // the block's first / last image row
        upM = hasU && top && wave == 0;
        dnM = hasD && bot && wave == 3;
        pu = pd = wave * 32 + li;
        if (hasU && !top) pu -= d.W;
        if (hasU && top && wave > 0) pu = (wave - 1) * 32 + (p.pool_rpb - 1) * d.W + ow;      // (a block above is a full one)
        if (hasD && !bot) pd += d.W;
        if (hasD && bot && wave < 3) pd = (wave + 1) * 32 + ow;
    }
    const int m = mrow0 + li;
    const unsigned voff = (item && m < Mw) ? ((unsigned)m * (unsigned)d.ldx + 4u * kh) * 4u : kOOB;

    // B DMA slots.  n-contiguous weights (forward): buffer layout [k][n], slot -> (k = idx / (BN/4), n4 = idx % (BN/4)).
    // k-contiguous weights (dgrad): buffer layout [n][16 k] with the four 16-byte chunks of a row XOR-swizzled by
    // (n >> 2) & 3 on the SOURCE side (the DMA destination is lane-linear), conflict-free for ds_read_b128.
    unsigned uoff[DJ];
    int ukq[DJ];
#pragma unroll
    for (int i = 0; i < DJ; ++i) {
        const int idx = i * 256 + tid;
        if (BNMAJOR) {
            const int k = idx / (BN / 4), n = n0 + (idx % (BN / 4)) * 4;
            ukq[i] = k;
            uoff[i] = (n < d.Cout && k < WK) ? ((unsigned)k * (unsigned)d.w_k_stride + (unsigned)n) * 4u : kOOB;
        } else {
            const int nl = idx >> 2, pc = idx & 3, kq = pc ^ ((nl >> 2) & 3);
            ukq[i] = kq * 4;
            uoff[i] = (n0 + nl < d.Cout && nl < BN) ? ((unsigned)(n0 + nl) * (unsigned)d.w_n_stride + 4u * kq) * 4u : kOOB;
        }
    }
    auto dma_b = [&](int buf, int c0, int i) {
        // past the end of the reduction the weights must read as zeros (the A operand there is whatever follows in
        // the row): out-of-range offset
        const bool ok = c0 + ukq[i] < K;
        const unsigned off = BNMAJOR ? uoff[i] + (unsigned)c0 * (unsigned)d.w_k_stride * 4u : uoff[i] + (unsigned)c0 * 4u;
        // (written as an if: hipcc's host pass silently dropped this kernel's stub with a `cond ? off : kOOB` here)
        unsigned o = off;
        if (!ok || uoff[i] == 0x80000000u) o = 0x80000000u;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(srd_w, (lds_ptr)(smem + buf * BSZ + wave * 256 + i * 1024), 16, o, 0, 0, 0);
    };

    f32x16 acc[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[b][e] = 0.f;

    // POOL: the rows above and below (out-of-range where they do not exist), the winners' bytes, the neighbour exchange
    const unsigned vup = (POOL && upM) ? voff - (unsigned)prow : kOOB, vdn = (POOL && dnM) ? voff + (unsigned)prow : kOOB;
    const __amdgpu_buffer_rsrc_t srd_am = make_srd(POOL ? (const void *)d.pool_argmax : (const void *)p.x,
                                                   POOL ? (unsigned)((int64_t)p.M * K) : 0u);
    const unsigned vam = (POOL && item && m < Mw && t0.col == 0) ? (unsigned)m * (unsigned)K + 8u * kh : kOOB;
    // POOL: the halo row of this wave -- the image row above wave 0's block or below wave 3's; waves 1 and 2 have none
    const bool halo = POOL && (wave == 0 || wave == 3);          // (uniform)
    const unsigned vhalo = wave == 0 ? vup : vdn;
    f32x4 rh0 = {0.f, 0.f, 0.f, 0.f}, rh1 = {0.f, 0.f, 0.f, 0.f};
    auto load_halo = [&](int c0) {
        if (halo) {
            rh0 = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(srd_x, vhalo, c0 * 4, 0));
            rh1 = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(srd_x, vhalo, c0 * 4 + 32, 0));
        }
    };
    // POOL: the centre rows of a K step, raw, as an LDS tile [2 stages][128 pixels][16 channels].  A wave fetches its block
    // with FOUR lanes per pixel (lane -> pixel 16 j + lane / 4, 16-byte chunk lane % 4: one 64-byte sector per quad, where the
    // fragment layout touches four rows per quad and the L1 spends a tag lookup on each), puts it into the tile, and every
    // wave reads its own fragments AND the pixels above and below from there: an input row is fetched once per workgroup.
    // The four chunks of a pixel are XOR-swizzled by (pixel >> 1) & 3 (conflict-free fragment reads).
    float *const ptile = smem + BST * BSZ + 256;
    const int pown = wave * 32 + li, sown = (li >> 1) & 3, sup = (pu >> 1) & 3, sdn = (pd >> 1) & 3;
    unsigned vco[2] = {kOOB, kOOB};
    int tco[2] = {0, 0};
    if constexpr (POOL) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int row = 16 * j + (lane >> 2), chunk = lane & 3;
            vco[j] = (item && mrow0 + row < Mw) ? ((unsigned)(mrow0 + row) * (unsigned)d.ldx + 4u * chunk) * 4u : kOOB;
            tco[j] = (wave * 32 + row) * 16 + ((chunk ^ ((row >> 1) & 3)) * 4);
        }
    }
    auto tile_put = [&](int st, const f32x4 &c0v, const f32x4 &c1v) {
        *reinterpret_cast<f32x4 *>(ptile + st * PT + tco[0]) = c0v;
        *reinterpret_cast<f32x4 *>(ptile + st * PT + tco[1]) = c1v;
    };
    auto tile_get = [&](int st, int px, int sw, int half) -> f32x4 {
        return *reinterpret_cast<const f32x4 *>(ptile + st * PT + px * 16 + (((2 * half + kh) ^ sw) * 4));
    };
    // lane i <- lane i - 1 / lane i + 1 of the wave (DPP wave shifts: one VALU move each, no LDS).  The block starts and ends
    // at image-row boundaries, so the lanes the shift wraps into (0, 31 | 32, 63) never use what they get.
    auto from_left = [](float v) -> float {
        return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x138 /* wave_shr:1 */, 0xf, 0xf, false));
    };
    auto from_right = [](float v) -> float {
        return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x130 /* wave_shl:1 */, 0xf, 0xf, false));
    };
    // c <- max over the 3x3 neighbourhood (c = the centre row's values), returns the four winners kh * 3 + kw as bytes:
    // column maximum and its FIRST row, then among the (up to) three columns that reach the overall maximum the smallest
    // kh * 3 + kw -- the first maximum in row-major order, maxpool3_fwd_rolling's rule
    auto pool4 = [&](f32x4 &c, const f32x4 &u, const f32x4 &dn) -> unsigned {
        unsigned bytes = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float uu = hasU ? u[j] : -INFINITY, dd = hasD ? dn[j] : -INFINITY;
            const float cm = fmaxf(fmaxf(uu, c[j]), dd);
            const int t = uu == cm ? 0 : (c[j] == cm ? 3 : 6);
            const float lraw = from_left(cm), rraw = from_right(cm);
            const int tl = __builtin_amdgcn_update_dpp(0, t, 0x138, 0xf, 0xf, false);
            const int tr = __builtin_amdgcn_update_dpp(0, t, 0x130, 0xf, 0xf, false);
            const float lv = hasL ? lraw : -INFINITY, rv = hasR ? rraw : -INFINITY;
            const float best = fmaxf(fmaxf(lv, cm), rv);
            const int il = lv == best ? tl : 99, ic = cm == best ? t + 1 : 99, ir = rv == best ? tr + 2 : 99;
            const int arg = min(min(il, ic), ir);
            c[j] = best;
            bytes |= (unsigned)arg << (8 * j);
        }
        return bytes;
    };
    f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = {0.f, 0.f, 0.f, 0.f};
    // the A loads of a K step: the lane's fragments, POOL: its two chunks of the tile
    const unsigned va0 = POOL ? vco[0] : voff, va1 = POOL ? vco[1] : voff;
    constexpr int kA1 = POOL ? 0 : 32;
    a0 = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(srd_x, va0, 0, 0));
    a1 = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(srd_x, va1, kA1, 0));
    if constexpr (POOL) load_halo(0);
    // BNB: the gradient dy of the layer's activation, per channel range its own descriptor and row offset
    const ds_bn_bwd_on_load &bb = p.bnb;
    __amdgpu_buffer_rsrc_t srd_dy[3];
    unsigned vdy[3];
    if (BNB) {
#pragma unroll
        for (int sg = 0; sg < 3; ++sg) {
            const bool has = sg < bb.nseg;
            const int cb = sg == 0 ? 0 : bb.c_end[sg - 1];
            const int ld = has ? bb.ld[sg] : 0;
            srd_dy[sg] = make_srd(has ? bb.dy[sg] : bb.dy[0], has ? (unsigned)(((int64_t)(p.M - 1) * ld + (bb.c_end[sg] - cb)) * 4) : 0u);
            vdy[sg] = (has && item && m < p.M) ? ((unsigned)m * (unsigned)ld + 4u * kh) * 4u : kOOB;
        }
    }
    auto load_dy = [&](int c0, int half) -> f32x4 {          // channels c0 + 8 half + 4 kh ... of the step that starts at c0
        const int sg = (c0 < bb.c_end[0] || bb.nseg == 1) ? 0 : ((c0 < bb.c_end[1] || bb.nseg == 2) ? 1 : 2);     // (uniform)
        const int cb = sg == 0 ? 0 : bb.c_end[sg - 1];
        const __amdgpu_buffer_rsrc_t r = sg == 0 ? srd_dy[0] : (sg == 1 ? srd_dy[1] : srd_dy[2]);
        const unsigned v = sg == 0 ? vdy[0] : (sg == 1 ? vdy[1] : vdy[2]);
        return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, v, (c0 - cb) * 4 + 32 * half, 0));
    };
    f32x4 d0 = {0.f, 0.f, 0.f, 0.f}, d1 = {0.f, 0.f, 0.f, 0.f};
    if (BNB) {
        d0 = load_dy(0, 0);
        d1 = load_dy(0, 1);
    }
#pragma unroll
    for (int i = 0; i < DJ; ++i) dma_b(0, 0, i);
    const int ksteps = (K + WK - 1) / WK;
    // x holds pre-BatchNorm conv outputs: the A fragment becomes relu(x * rstd[k] + shift[k]) as it is loaded (two
    // packed multiply-adds and two packed max per float4, against 4 NB MFMAs); channels past Cin get (0, 0) -> 0
    const bool norm = d.norm_rstd != nullptr;          // (uniform)
    if (norm) {
        for (int c = tid; c < ksteps * WK; c += 256) {
            nrm[0][c] = c < K ? d.norm_rstd[c] : 0.f;
            nrm[1][c] = c < K ? d.norm_shift[c] : 0.f;
        }
    }
    auto apply_norm = [&](f32x4 &a, int c) {           // channels c .. c + 3
        const f32x4 r = *reinterpret_cast<const f32x4 *>(&nrm[0][c]), sh = *reinterpret_cast<const f32x4 *>(&nrm[1][c]);
        const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
        a = __builtin_elementwise_max(__builtin_elementwise_fma(a, r, sh), zero);
    };
    if (BNB) {          // channels past Cin get zeros: dz = 0 there (and the weights read as zeros anyway)
        for (int c = tid; c < ksteps * WK; c += 256) {
            nrm[0][c] = c < K ? bb.rstd[c] : 0.f;
            nrm[1][c] = c < K ? bb.shift[c] : 0.f;
            nrm[BNB ? 2 : 0][c] = c < K ? bb.mean[c] : 0.f;
            nrm[BNB ? 3 : 0][c] = c < K ? bb.coef[c] : 0.f;
            nrm[BNB ? 4 : 0][c] = c < K ? bb.coef[K + c] : 0.f;
        }
    }
    auto apply_bnb = [&](f32x4 &a, const f32x4 &dy, int c) {      // a holds z of channels c .. c + 3
        const f32x4 r = *reinterpret_cast<const f32x4 *>(&nrm[0][c]), sh = *reinterpret_cast<const f32x4 *>(&nrm[1][c]);
        const f32x4 mu = *reinterpret_cast<const f32x4 *>(&nrm[BNB ? 2 : 0][c]);
        const f32x4 k1 = *reinterpret_cast<const f32x4 *>(&nrm[BNB ? 3 : 0][c]), k2 = *reinterpret_cast<const f32x4 *>(&nrm[BNB ? 4 : 0][c]);
#pragma unroll
        for (int j = 0; j < 4; ++j) a[j] = ds::bn_bwd_dz(a[j], dy[j], r[j], sh[j], mu[j], k1[j], k2[j]);
    };
    if constexpr (POOL) tile_put(0, a0, a1);
    __syncthreads();
    // stage st of the tile holds every wave's centre rows of channels c0 ...: a0 / a1 <- the lane's fragments pooled, and
    // the winners recorded
    // The operands of the step after it (channels cnext ..., none: cnext < 0) are requested from here, behind the barrier
    // that made the tile visible and ahead of the pooling arithmetic: they have that and the step's MFMAs to arrive.
    f32x4 pn0 = {0.f, 0.f, 0.f, 0.f}, pn1 = {0.f, 0.f, 0.f, 0.f};
    auto pool_step = [&](int c0, int st, int cnext) {
        if (cnext >= 0) {
            pn0 = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(srd_x, va0, cnext * 4, 0));
            pn1 = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(srd_x, va1, cnext * 4, 0));
        }
        a0 = tile_get(st, pown, sown, 0);
        a1 = tile_get(st, pown, sown, 1);
        f32x4 u0 = tile_get(st, pu, sup, 0), u1 = tile_get(st, pu, sup, 1);
        f32x4 e0 = tile_get(st, pd, sdn, 0), e1 = tile_get(st, pd, sdn, 1);
        if (halo) {
            if (wave == 0) {
                u0 = upM ? rh0 : u0;
                u1 = upM ? rh1 : u1;
            } else {
                e0 = dnM ? rh0 : e0;
                e1 = dnM ? rh1 : e1;
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        if (cnext >= 0) load_halo(cnext);          // (this step's halo is in u / e now)
        __builtin_amdgcn_sched_barrier(0);
        const unsigned w0 = pool4(a0, u0, e0), w1 = pool4(a1, u1, e1);
        // the lanes (pixel, 0) and (pixel, 1) trade a word: 8 consecutive winners per lane, one store per K step
        const auto sw = __builtin_amdgcn_permlane32_swap(w0, w1, false, false);
        typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
        const u32x2 pr = {sw[0], sw[1]};
        __builtin_amdgcn_raw_buffer_store_b64(pr, srd_am, vam, c0, 0);
    };
    if constexpr (POOL) pool_step(0, 0, ksteps > 1 ? WK : -1);
    if (norm) {
        apply_norm(a0, 4 * kh);
        apply_norm(a1, 8 + 4 * kh);
    }
    if (BNB) {
        apply_bnb(a0, d0, 4 * kh);
        apply_bnb(a1, d1, 8 + 4 * kh);
    }
    for (int ks = 0; ks < ksteps; ++ks) {
        const bool more = ks + 1 < ksteps;
        const int cn = (ks + 1) * WK;
        const float *b_s = smem + (ks & 1) * BSZ;
        f32x4 n0v = a0, n1v = a1;
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            // B fragments of column block b: lane (n, kh) needs B[k = 4 kh + j (+ 8)][32 b + n]
            float bf[8];
            if (BNMAJOR) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    bf[j] = b_s[(4 * kh + j) * BN + 32 * b + li];
                    bf[4 + j] = b_s[(8 + 4 * kh + j) * BN + 32 * b + li];
                }
            } else {
                const int nl = 32 * b + li, sw = (nl >> 2) & 3;
                const f32x4 lo = *reinterpret_cast<const f32x4 *>(b_s + nl * 16 + ((kh ^ sw) * 4));
                const f32x4 hi = *reinterpret_cast<const f32x4 *>(b_s + nl * 16 + (((2 + kh) ^ sw) * 4));
#pragma unroll
                for (int j = 0; j < 4; ++j) { bf[j] = lo[j]; bf[4 + j] = hi[j]; }
            }
            if (more) {                                    // next K step's operands, spread over the column blocks
                if (b == 0 && !POOL) {                     // (POOL: requested by the pool step, see there)
                    n0v = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(srd_x, voff, cn * 4, 0));
                    if (BNB) d0 = load_dy(cn, 0);
                }
                if (b == ((NB > 1 && !DS_WIDE_A_B2B) ? 1 : 0) && !POOL) {
                    n1v = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(srd_x, voff, cn * 4 + 32, 0));
                    if (BNB) d1 = load_dy(cn, 1);
                }
                if (b < DJ) dma_b((ks + 1) & 1, cn, b);
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[j], bf[j], acc[b], 0, 0, 0);
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[j], bf[4 + j], acc[b], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
        }
        if (more && DJ > NB) {
#pragma unroll
            for (int i = NB; i < DJ; ++i) dma_b((ks + 1) & 1, cn, i);
        }
        if constexpr (POOL) {
            // the K step's barrier stands between the waves' puts and their reads of the tile, whose other stage the slower
            // waves may still be reading
            if (more) tile_put((ks + 1) & 1, pn0, pn1);
            __syncthreads();
            if (more) pool_step(cn, (ks + 1) & 1, ks + 2 < ksteps ? cn + WK : -1);
        } else {
            a0 = n0v;
            a1 = n1v;
        }
        if (norm && more) {
            apply_norm(a0, cn + 4 * kh);
            apply_norm(a1, cn + 8 + 4 * kh);
        }
        if (BNB && more) {
            apply_bnb(a0, d0, cn + 4 * kh);
            apply_bnb(a1, d1, cn + 8 + 4 * kh);
        }
        if constexpr (!POOL) __syncthreads();
    }

    // ---- epilogue (conv_epilogue.h): store, BatchNorm column statistics ------------------------------------------------
    // POOL: the row bound is this wave's last real row (Mw, wave-uniform), so the rows a 28-pixel block leaves unused -- they
    // would alias the NEXT block's pixels -- are dropped by the same range check as the rows past M; a surplus wave past the
    // last image has no row.
    float *red = smem + BST * BSZ;
    ds::wave_row_epilogue<NB, WideEpi<BNR>>(acc, d, p.z, p.mask, p.stats, p.pivot, item, n0, mrow0, Mw, Mw > mrow0, t0.row, t0.stride,
                                            red, wave, li, kh, p.scale, p.shift);
}


// ================================================================================================
// bf16 register-direct implicit GEMM (ds_conv_bf16): v_mfma_f32_32x32x16_bf16, fp32 accumulate, fp32 storage.
//
// Second generation of the DS_DTYPE_BF16 path (conv_bf16_kernel above stages both operands through registers AND
// LDS one K-tile ahead: 184 TFLOP/s, every fetch latency exposed against 256 matrix cycles).  Here:
//   * the weights are converted ONCE per weight update into the kernel's own order (ds_weights_to_bf16):
//     wb[it][column][16 k] bf16 with it = channel chunk * taps + tap -- exactly the K-loop order -- zero padded in k, so
//     the B operand of a step (four (chunk, tap) iterations x NB*32 columns x 16 k = NB * 4 KB) is a linear run that
//     LDS-DMA drops into LDS in fragment layout; no conversion, no transpose, no K-tail logic in the loop;
//   * the A operand is register-direct: lane (i, kh) of the 32x32x16 MFMA loads channels 8 kh .. 8 kh + 7 of ITS
//     pixel at the current tap as two float4 (SRD loads; padding pixels and rows past M read zeros from an
//     out-of-range offset), rounds them to bf16 (v_cvt_pk_bf16_f32, RNE) and that IS its A fragment;
//   * a wave owns 32 pixels x NB*32 columns (NB <= 8: 128 accumulator registers, two waves per SIMD); each A
//     fragment feeds NB MFMAs; the next step's eight A loads and NB weight DMAs are issued between the MFMA groups.
// Epilogue: fp32 stores + BatchNorm column statistics about the pivot (flags 0 or DS_EPI_STATS).
// ================================================================================================
// X3 (ds_conv_f32x3): fp32 PRODUCTS on the bf16 matrix cores.  Every fp32 operand is the sum of three bf16 pieces
// (8 + 8 + 8 mantissa bits: a = a0 + a1 + a2 exactly to 2^-24 |a|); a*b is accumulated in fp32 as
// a1*b1 + a2*b0 + a0*b2 + a1*b0 + a0*b1 + a0*b0 (the dropped terms are below 2^-24 |ab|): six v_mfma_f32_32x32x16_bf16
// (8 passes each) per 16 reduction channels and 32x32 tile instead of eight v_mfma_f32_32x32x2_f32 (16 passes each), i.e.
// 2.67x fewer matrix cycles at the accuracy of the fp32 MFMA (scripts/microbench/mfma_x3.hip: relative rms error against fp64
// 3.26e-7 vs 3.22e-7 over K = 512; loop 1.6 - 1.9x faster including the splitting).  The weights are split once per
// weight update (ds_weights_to_f32x3: three planes per K-loop iteration), the A fragment in registers (~40 VALU per 8
// values, shared by the NB column blocks).  Measured on the 1x1 layers of the joint step (B = 256): 1.15 - 1.5x over the
// wide fp32 kernel on twelve of fourteen shapes, up to 163 TFLOP/s of fp32-accurate GEMM -- above the fp32 MFMA peak.
struct Bf16dEpi : ds::WaveRowOpt { static constexpr bool half = true, mask_rstd = true; };

template <int NB, int KS, bool XB, bool X3 = false>      // KS x KS taps (1 or 3); XB: x is stored as bf16 (16-bit activation storage)
__global__ __launch_bounds__(256, 2) void conv_bf16d_kernel(const ConvParams p) {
    // iterations per step: X3 keeps three weight planes in LDS, so shorter steps (SI * NB % 4 == 0: whole DMA slots)
    constexpr int BN = NB * 32, SI = !X3 ? 4 : NB == 1 ? 4 : NB <= 4 ? 2 : 1, TAPS = KS * KS;
    constexpr int PL = X3 ? 3 : 1;                             // weight planes per iteration (X3: the three bf16 pieces)
    constexpr int NSL = SI * PL * NB / 4;                      // 16-byte DMA slots per thread and step
    static_assert(SI * PL * NB % 4 == 0, "a step's weight tile must be whole 256-lane DMA instructions");
    constexpr int BSZ = SI * PL * BN * 16;                     // bf16 elements per B buffer
    static_assert(!(X3 && XB), "ds_conv_f32x3 reads fp32 activations");
    __shared__ __attribute__((aligned(128))) __bf16 smem[2 * BSZ + 512];
    // X3 + ds_conv_desc.norm_rstd / norm_shift (1x1 only): x holds pre-BatchNorm values, relu(x*rstd + shift) on load
    __shared__ __attribute__((aligned(16))) float nrm[2][X3 ? 1024 + 16 : 4];
    const ds_conv_desc &d = p.d;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 31, kh = lane >> 5;
    const TileId t0 = tile_id(p);
    const int n0 = t0.col * BN;
    const bool item = t0.row < p.row_tiles;
    const __amdgpu_buffer_rsrc_t srd_x = make_srd(p.x, p.x_bytes);
    const __amdgpu_buffer_rsrc_t srd_w = make_srd(p.w, p.w_bytes);
    const int chunks = (d.Cin + 15) >> 4;
    const int iters = chunks * TAPS;
    const int nsteps = (iters + SI - 1) / SI;

    // ---- this lane's pixel and the byte offset of its input pixel at every tap (channel 8 kh) -----------------------
    const int m = t0.row * 128 + wave * 32 + li;
    const bool rv = item && m < p.M;
    const int ohw = d.OH * d.OW;
    const int n = (rv ? m : 0) / ohw;
    const int r = (rv ? m : 0) - n * ohw;
    const int oh = r / d.OW, ow = r - oh * d.OW;
    unsigned voff[TAPS];
#pragma unroll
    for (int a = 0; a < KS; ++a)
#pragma unroll
        for (int b = 0; b < KS; ++b) {
            const int ih = oh * d.stride - d.pad_t + a, iw = ow * d.stride - d.pad_l + b;
            const bool ok = rv && (unsigned)ih < (unsigned)d.H && (unsigned)iw < (unsigned)d.W;
            voff[a * KS + b] = ok ? ((unsigned)((n * d.H + ih) * d.W + iw) * (unsigned)d.ldx + 8u * kh) * (XB ? 2u : 4u) : kOOB;
        }
    // ---- B DMA slots of a step: slot -> (local iteration, column, 8-k half); source is linear in wb ---------------
    const int ncols = p.col_total;                              // columns of wb (Cout rounded up to 32)
    unsigned uoff[NSL];
    int uit[NSL];
#pragma unroll
    for (int i = 0; i < NSL; ++i) {
        const int sl = i * 256 + tid;
        const int itl = sl / (BN * 2), nn = (sl >> 1) % BN, half = sl & 1;
        uit[i] = itl;
        uoff[i] = (n0 + nn < ncols) ? ((unsigned)((itl * ncols + n0 + nn) * 16 + 8 * half)) * 2u : kOOB;
    }
    const unsigned it_bytes = (unsigned)ncols * 32u;            // bytes of one iteration's weights
    auto dma_b = [&](int buf, int step, int i) {
        unsigned o = uoff[i] + (unsigned)(step * SI * PL) * it_bytes;
        if (step * SI * PL + uit[i] >= iters * PL || uoff[i] == 0x80000000u) o = 0x80000000u;     // past the reduction: zeros
        __builtin_amdgcn_raw_ptr_buffer_load_lds(srd_w, (lds_ptr)(smem + buf * BSZ + wave * 512 + i * 2048), 16, o, 0, 0, 0);
    };
    // A loads of one (chunk, tap) iteration
    auto load_a = [&](int it, f32x4 &lo, f32x4 &hi) {
        const int chunk = it / TAPS, tap = it - chunk * TAPS;
        unsigned vo = voff[0];
#pragma unroll
        for (int k = 1; k < TAPS; ++k) vo = tap == k ? voff[k] : vo;
        if (XB) {           // eight bf16 channels = one 16-byte load, already the fragment
            lo = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(srd_x, vo, chunk * 32, 0));
        } else {
            lo = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(srd_x, vo, chunk * 64, 0));
            hi = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(srd_x, vo, chunk * 64 + 16, 0));
        }
    };

    f32x16 acc[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[b][e] = 0.f;

    f32x4 alo[SI], ahi[SI];
#pragma unroll
    for (int j = 0; j < SI; ++j) load_a(j, alo[j], ahi[j]);
#pragma unroll
    for (int i = 0; i < NSL; ++i) dma_b(0, 0, i);
    bool norm = false;
    if constexpr (X3) {
        norm = d.norm_rstd != nullptr;          // (uniform)
        if (norm)
            for (int c = tid; c < chunks * 16; c += 256) {
                nrm[0][c] = c < d.Cin ? d.norm_rstd[c] : 0.f;
                nrm[1][c] = c < d.Cin ? d.norm_shift[c] : 0.f;
            }
    }
    __syncthreads();
    for (int st = 0; st < nsteps; ++st) {
        const bool more = st + 1 < nsteps;
        const __bf16 *b_s = smem + (st & 1) * BSZ + li * 16 + kh * 8;
        f32x4 nlo[SI], nhi[SI];
#pragma unroll
        for (int j = 0; j < SI; ++j) {
            // A fragment: 8 consecutive channels rounded to bf16 (X3: split into three bf16 pieces)
            bf16x8 af, af1, af2;
            if (XB) {
                af = __builtin_bit_cast(bf16x8, alo[j]);
            } else {
                f32x4 xl = alo[j], xh = ahi[j];
                if constexpr (X3) {
                    if (norm) {
                        const int c = ((st * SI + j) / TAPS) * 16 + 8 * kh;
                        const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
                        xl = __builtin_elementwise_max(__builtin_elementwise_fma(xl, *reinterpret_cast<const f32x4 *>(&nrm[0][c]),
                                                                                 *reinterpret_cast<const f32x4 *>(&nrm[1][c])), zero);
                        xh = __builtin_elementwise_max(__builtin_elementwise_fma(xh, *reinterpret_cast<const f32x4 *>(&nrm[0][c + 4]),
                                                                                 *reinterpret_cast<const f32x4 *>(&nrm[1][c + 4])), zero);
                    }
                }
                bf16x4 l4 = __builtin_convertvector(xl, bf16x4), h4 = __builtin_convertvector(xh, bf16x4);
                af = __builtin_shufflevector(l4, h4, 0, 1, 2, 3, 4, 5, 6, 7);
                if constexpr (X3) {
                    xl -= __builtin_convertvector(l4, f32x4);
                    xh -= __builtin_convertvector(h4, f32x4);
                    l4 = __builtin_convertvector(xl, bf16x4);
                    h4 = __builtin_convertvector(xh, bf16x4);
                    af1 = __builtin_shufflevector(l4, h4, 0, 1, 2, 3, 4, 5, 6, 7);
                    xl -= __builtin_convertvector(l4, f32x4);
                    xh -= __builtin_convertvector(h4, f32x4);
                    af2 = __builtin_shufflevector(__builtin_convertvector(xl, bf16x4), __builtin_convertvector(xh, bf16x4), 0, 1, 2, 3, 4, 5, 6, 7);
                }
            }
            if (more) {             // next step's operands between the MFMA groups
                load_a((st + 1) * SI + j, nlo[j], nhi[j]);
#pragma unroll
                for (int i = j; i < NSL; i += SI) dma_b((st + 1) & 1, st + 1, i);
            }
            bf16x8 bfr[PL][NB];
#pragma unroll
            for (int pl = 0; pl < PL; ++pl)
#pragma unroll
                for (int b = 0; b < NB; ++b) bfr[pl][b] = *reinterpret_cast<const bf16x8 *>(b_s + ((j * PL + pl) * BN + b * 32) * 16);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int b = 0; b < NB; ++b) {
                if constexpr (X3) {         // small terms first
                    acc[b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af1, bfr[1][b], acc[b], 0, 0, 0);
                    acc[b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af2, bfr[0][b], acc[b], 0, 0, 0);
                    acc[b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, bfr[PL - 1][b], acc[b], 0, 0, 0);
                    acc[b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af1, bfr[0][b], acc[b], 0, 0, 0);
                    acc[b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, bfr[PL > 1 ? 1 : 0][b], acc[b], 0, 0, 0);
                }
                acc[b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, bfr[0][b], acc[b], 0, 0, 0);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int j = 0; j < SI; ++j) { alo[j] = nlo[j]; ahi[j] = nhi[j]; }
        __syncthreads();
    }

    // ---- epilogue (conv_epilogue.h): store, BatchNorm column statistics; 16-bit z / activation storage per launch ---------
    ds::wave_row_epilogue<NB, Bf16dEpi>(acc, d, p.z, p.mask, p.stats, p.pivot, item, n0, t0.row * 128 + wave * 32, p.M, true, t0.row,
                                        t0.stride, reinterpret_cast<float *>(smem + 2 * BSZ), wave, li, kh, nullptr, nullptr);
}

// wb[it][column][16] bf16, it = chunk * taps + tap, from the TF HWIO filter w [taps][Cin][Cout] (fp32).
//   dgrad == 0: column = co, k = ci (forward);  dgrad == 1: column = ci, k = co, taps flipped (Conv2DBackpropInput).
// Columns are padded to a multiple of 32 and k to a multiple of 16 with zeros.
__global__ __launch_bounds__(256) void weights_to_bf16_kernel(const float *w, __bf16 *wb, int Cin, int Cout, int taps,
                                                              int dgrad) {
    const int K = dgrad ? Cout : Cin, Ncol = dgrad ? Cin : Cout;
    const int chunks = (K + 15) >> 4, ncols = (Ncol + 31) / 32 * 32;
    const int64_t total = (int64_t)chunks * taps * ncols * 16;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int j = (int)(i & 15);
        const int64_t rest = i >> 4;
        const int col = (int)(rest % ncols);
        const int it = (int)(rest / ncols);
        const int chunk = it / taps, tap = it - chunk * taps;
        const int k = chunk * 16 + j;
        float v = 0.f;
        if (col < Ncol && k < K) {
            const int ci = dgrad ? col : k, co = dgrad ? k : col, tp = dgrad ? taps - 1 - tap : tap;
            v = w[((int64_t)tp * Cin + ci) * Cout + co];
        }
        wb[i] = (__bf16)v;
    }
}

// the three bf16 pieces of every weight, in the K-loop order of conv_bf16d_kernel<.., X3>: [iteration][piece][column][16 k]
__global__ __launch_bounds__(256) void weights_to_f32x3_kernel(const float *w, __bf16 *wb, int Cin, int Cout, int taps,
                                                               int dgrad) {
    const int K = dgrad ? Cout : Cin, Ncol = dgrad ? Cin : Cout;
    const int chunks = (K + 15) >> 4, ncols = (Ncol + 31) / 32 * 32;
    const int64_t total = (int64_t)chunks * taps * ncols * 16;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int j = (int)(i & 15);
        const int64_t rest = i >> 4;
        const int col = (int)(rest % ncols);
        const int it = (int)(rest / ncols);
        const int chunk = it / taps, tap = it - chunk * taps;
        const int k = chunk * 16 + j;
        float v = 0.f;
        if (col < Ncol && k < K) {
            const int ci = dgrad ? col : k, co = dgrad ? k : col, tp = dgrad ? taps - 1 - tap : tap;
            v = w[((int64_t)tp * Cin + ci) * Cout + co];
        }
        const __bf16 p0 = (__bf16)v;
        const float r1 = v - (float)p0;
        const __bf16 p1 = (__bf16)r1;
        const __bf16 p2 = (__bf16)(r1 - (float)p1);
        const int64_t o = (((int64_t)it * 3) * ncols + col) * 16 + j;
        wb[o] = p0;
        wb[o + (int64_t)ncols * 16] = p1;
        wb[o + (int64_t)ncols * 32] = p2;
    }
}

// ---- host-side dispatch -----------------------------------------------------------------------
typedef void (*KernelFn)(const ConvParams);

int64_t conv_M(const ds_conv_desc *d) { return (int64_t)d->N * d->OH * d->OW; }

// f(std::integral_constant<int, n>) with n = the runtime i in LO .. HI (values beyond an end take that end): turns a tile or
// block count into the template argument of a kernel
template <int LO, int HI, class F>
KernelFn with_const(int i, F &&f) {
    if constexpr (LO < HI)
        if (i > LO) return with_const<LO + 1, HI>(i, f);
    return f(std::integral_constant<int, LO>{});
}

// The tuning state of the selection rules.  The DS_* knobs are read once through ds::tune_env (the product build reads no
// environment, so every knob keeps its default there); the ds_debug_conv_* switches of the tuning build write into it.
struct Tuning {
    int wide = 1;             // DS_CONV_WIDE / ds_debug_conv_set_wide, A/B aid: 0 = never, 1 = automatic, 2 = wherever the shape allows
    int wide_cost = 0;        // DS_WIDE_COST: the A fetch in wide_nb's cost, in halves of a block
    int wide_nb = 0;          // DS_WIDE_NB pins the wide kernel's column blocks per wave
    int wide_min_wgs = 128;   // DS_WIDE_MINWGS (see wide_nb)
    int mt = 0, nt = 0;       // DS_CONV_CFG="mt,nt" / ds_debug_conv_set_tile pin the tile
    int path = 0;             // DS_CONV_PATH=lds|glds / ds_debug_conv_set_path pin the kernel family: 1 / 3
    int prio = 0;             // DS_CONV_PRIO; opt-in: measured neutral-to-negative (profiles/r01_notes.md)
    int xcd_remap = 1;        // DS_CONV_XCD_REMAP, A/B aid; default on
    int bf16d_max_nb = 8;     // ds_debug_conv_bf16_set_max_nb
};

Tuning &tuning() {
    static Tuning tune = [] {
        Tuning t;
        const auto knob = [](const char *name, int *v) {
            if (const char *e = ds::tune_env(name)) *v = atoi(e);
        };
        knob("DS_CONV_WIDE", &t.wide);
        knob("DS_WIDE_COST", &t.wide_cost);
        knob("DS_WIDE_NB", &t.wide_nb);
        knob("DS_WIDE_MINWGS", &t.wide_min_wgs);
        knob("DS_CONV_PRIO", &t.prio);
        knob("DS_CONV_XCD_REMAP", &t.xcd_remap);
        if (const char *e = ds::tune_env("DS_CONV_CFG")) sscanf(e, "%d,%d", &t.mt, &t.nt);
        if (const char *e = ds::tune_env("DS_CONV_PATH")) t.path = e[0] == 'l' ? 1 : (e[0] == 'g' ? 3 : 0);
        return t;
    }();
    return tune;
}

struct TileCfg {
    int mt, nt;
    bool glds;       // LDS-DMA kernel, K-tile 32 (128 x 32*nt tile)
    bool bf16;       // bf16-multiply kernel (128 x 32*nt tile, nt <= 4)
    int wide;        // > 0: wide 1x1 kernel, 128 rows x 32*wide columns per workgroup
};

struct Variant {
    bool bnmajor, fold, vec;
};

// A plan-time question may be put before the operand it is about is attached to the descriptor
enum Ask { kAsIs, kBeforeBnb, kBeforePool };

// Everything ds_conv_igemm's launch of a descriptor is: made by choose(), consumed by igemm_launch, ds_gemm_group and the
// plan-time questions
struct Launch {
    Variant v;
    TileCfg c;
    bool bnr, pool, bnb;      // DS_EPI_BN_RELU / pool_argmax / bnb instantiation
    int row_tiles, gx, gy;    // row tiles, workgroups along the rows, column tiles
    bool one;                 // one workgroup per tile
    dim3 grid;                // the launch's grid (z = split-K slices) ...
    int col_tiles;            // ... and ConvParams.col_tiles: > 0 for the 1-D XCD-aware shape (TileId)
    int partials;             // statistics partials per channel the launch writes
};

// vector (16-byte) loads are legal when every stride is a multiple of 4 floats; pointer alignment is
// checked separately at launch
bool dims_vec(const ds_conv_desc *d) {
    const bool bnmajor = d->w_n_stride == 1 && d->w_k_stride != 1;
    const bool a_vec = (d->ldx % 4 == 0) && (d->Cin % 4 == 0);
    const bool b_vec = bnmajor ? (d->Cout % 4 == 0) && (d->w_k_stride % 4 == 0) && (d->w_tap_stride % 4 == 0)
                               : (d->Cin % 4 == 0) && (d->w_n_stride % 4 == 0) && (d->w_tap_stride % 4 == 0);
    return a_vec && b_vec;
}

bool aligned16(const void *x, const void *w) { return (((uintptr_t)x | (uintptr_t)w) & 15) == 0; }

// The kernel of a launch choice: every instantiation of the library's conv kernels is named here, in ds_conv_bf16 or in
// ds_conv_f32x3.
KernelFn kernel_of(const Launch &L) {
    const TileCfg &c = L.c;
    const Variant &v = L.v;
    if (c.wide) {
        if (L.bnr) {          // (bnr_ok: forward, no bnb)
            if (L.pool)
                return with_const<1, 4>(c.wide, [](auto nb) { return gemm_wide_kernel<decltype(nb)::value, true, false, true, true>; });
            return with_const<1, 8>(c.wide, [](auto nb) { return gemm_wide_kernel<decltype(nb)::value, true, false, false, true>; });
        }
        if (L.pool)          // (pool3_nb: forward, one column tile of at most four blocks)
            return with_const<1, 4>(c.wide, [](auto nb) { return gemm_wide_kernel<decltype(nb)::value, true, false, true>; });
        if (L.bnb)          // (wide_nb: at most two column blocks per wave with ds_conv_desc.bnb)
            return with_const<1, 2>(c.wide, [](auto nb) { return gemm_wide_kernel<decltype(nb)::value, false, true>; });
        return with_const<1, 8>(c.wide, [&](auto nb) {
            return v.bnmajor ? gemm_wide_kernel<decltype(nb)::value, true> : gemm_wide_kernel<decltype(nb)::value, false>;
        });
    }
    if (L.bnr) {          // DS_EPI_BN_RELU instantiations: forward (n-contiguous weights), 16-byte loads, 128-row tiles
        if (c.glds) return with_const<1, 3>(c.nt, [](auto nt) { return conv_glds_kernel<decltype(nt)::value, true, true>; });
        return with_const<1, 6>(c.nt, [](auto nt) { return conv_igemm_kernel<1, decltype(nt)::value, true, false, true, true>; });
    }
    if (c.bf16)
        return with_const<1, 4>(c.nt, [&](auto nt) {
            constexpr int NT = decltype(nt)::value;
            if (v.fold) return conv_bf16_kernel<NT, true, true>;
            return v.bnmajor ? conv_bf16_kernel<NT, true, false> : conv_bf16_kernel<NT, false, false>;
        });
    if (c.glds)
        return with_const<1, 3>(c.nt, [&](auto nt) {
            return v.bnmajor ? conv_glds_kernel<decltype(nt)::value, true> : conv_glds_kernel<decltype(nt)::value, false>;
        });
    return with_const<1, 2>(c.mt == 2 ? 2 : 1, [&](auto mt) {
        constexpr int MT = decltype(mt)::value;
        return with_const<1, 6>(c.nt, [&](auto nt) {
            constexpr int NT = decltype(nt)::value;
            if (v.bnmajor) {
                if (v.fold) return conv_igemm_kernel<MT, NT, true, true, true>;
                return v.vec ? conv_igemm_kernel<MT, NT, true, false, true> : conv_igemm_kernel<MT, NT, true, false, false>;
            }
            return v.vec ? conv_igemm_kernel<MT, NT, false, false, true> : conv_igemm_kernel<MT, NT, false, false, false>;
        });
    });
}

// MaxPool 3x3/1 on load (ds_conv_desc.pool_argmax): forward 1x1 conv with n-contiguous weights on a map at most 32 wide
// (a wave's 32-row block holds whole image rows), whole 16-channel K steps, ONE column tile of at most four blocks (the
// pooling is the loader's work and would be redone per column tile).  Returns the column blocks per wave, 0 = unsupported.
int pool3_nb(const ds_conv_desc *d, bool vec) {
    if (!vec || d->dtype != DS_DTYPE_F32) return 0;
    if (d->KH != 1 || d->KW != 1 || d->stride != 1 || d->fold_cin || d->splits > 1 || d->bnb) return 0;
    if (d->flags & ~(DS_EPI_STATS | DS_EPI_BN_RELU)) return 0;
    if (!(d->w_n_stride == 1 && d->w_k_stride != 1)) return 0;
    if (d->W > 32 || d->Cin % 16 != 0 || d->Cin < 16 || d->Cin > 1024 || d->Cout > 128) return 0;
    const int64_t M = conv_M(d);
    if (((M - 1) * d->ldz + d->Cout) * 4 >= (1ll << 31) || M * d->Cin >= (1ll << 31)) return 0;
    return (d->Cout + 31) / 32;
}

// POOL: image rows per 32-pixel block and blocks per image
void pool3_blocks(const ds_conv_desc *d, int *rpb, int *bpi) {
    *rpb = 32 / d->W;
    *bpi = (d->H + *rpb - 1) / *rpb;
}

// Column blocks per wave of the wide 1x1 kernel for `d`, or 0 when the layer stays on the LDS-tile kernels:
// plain 1x1 stride-1 GEMM shape, flags within {STATS}, vector-aligned, no split-K, enough workgroups to fill the chip.
int wide_nb(const ds_conv_desc *d, bool vec, Ask ask) {
    if (d->pool_argmax || ask == kBeforePool) return pool3_nb(d, vec);
    const Tuning &t = tuning();
    if (!t.wide || !vec || d->dtype != DS_DTYPE_F32) return 0;
    if (d->KH != 1 || d->KW != 1 || d->stride != 1 || d->fold_cin || d->splits > 1) return 0;
    if (d->flags & ~(DS_EPI_STATS | DS_EPI_ACCUM | DS_EPI_BNSUMS | DS_EPI_BN_RELU)) return 0;
    if (d->Cin % 8 != 0 || d->Cin < 32) return 0;
    const int64_t M = conv_M(d);
    // the epilogue addresses z (and the BatchNorm-sums activation) through 32-bit buffer offsets
    if (((M - 1) * d->ldz + d->Cout) * 4 >= (1ll << 31)) return 0;
    if ((d->flags & DS_EPI_BNSUMS) && ((M - 1) * d->ldmask + d->Cout) * 4 >= (1ll << 31)) return 0;
    const int N = d->Cout;
    // Every workgroup puts one wave on each SIMD of its CU and the resident waves of a SIMD share its matrix pipe, so a
    // launch takes ceil(workgroups / CUs) x (one wave's work): NB blocks of MFMAs per K step plus about half a block
    // for the A fetch it does not share.  Pick the NB with the least of that (ties to the wider tile).
    int best = 0, best_pad = 0;
    int64_t best_cost = (int64_t)1 << 60;
    const int64_t row_tiles = (M + 127) / 128;
    // (BatchNorm backward on load is kept for narrow dgrads only -- it wins on Conv2d_2b and nowhere else,
    // profiles/r04_bnb_layers.txt -- so its loader is instantiated for one and two column blocks per wave)
    const int nb_max = (d->bnb || ask == kBeforeBnb) ? 2 : 8;
    for (int nb = nb_max; nb >= (N <= 32 ? 1 : 2); --nb) {      // one block per wave only where two would be half padding
        const int tiles = (N + 32 * nb - 1) / (32 * nb);
        const int64_t rounds = (row_tiles * tiles + ds::kCUs - 1) / ds::kCUs;
        const int64_t cost = rounds * (2 * nb + t.wide_cost);
        if (cost < best_cost) { best_cost = cost; best = nb; best_pad = tiles * 32 * nb; }
    }
    if (t.wide_nb >= 1 && t.wide_nb <= nb_max) {
        best = t.wide_nb;
        best_pad = (N + 32 * best - 1) / (32 * best) * 32 * best;
    }
    const int64_t wgs = row_tiles * ((N + 32 * best - 1) / (32 * best));
    // measured per shape (profiles/r02_wide_layers.txt): wins 1.1-1.4x except with one mostly padded column tile or too
    // few workgroups to cover the CUs (7x7 maps with N <= 128)
    if (t.wide < 2 && (wgs < t.wide_min_wgs || best_pad * 100 > N * 125)) return 0;
    return best;
}

// Resident workgroups per CU of one instantiation (register/LDS limited), queried once and cached.
// The persistent grid is sized to exactly one resident wave of workgroups so no CU idles while a
// partial second wave runs; correctness never depends on it (no inter-workgroup communication).
int resident_per_cu(KernelFn kernel) {
    static std::unordered_map<const void *, int> cache;
    static std::mutex guard;          // (plans are made from one thread per device)
    const std::lock_guard<std::mutex> lock(guard);
    int &slot = cache[(const void *)kernel];
    if (slot == 0) {
        int n = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, (const void *)kernel, 256, 0) != hipSuccess || n < 1) n = 1;
        slot = n > 8 ? 8 : n;
    }
    return slot;
}

TileCfg pick_cfg(const ds_conv_desc *d, bool vec, Ask ask) {
    const Tuning &t = tuning();
    const int64_t M = conv_M(d);
    const int N = d->Cout;
    const int pad32 = (N + 31) / 32 * 32, pad64 = (N + 63) / 64 * 64;
    TileCfg c = {1, 1, false, false, 0};
    if (int nb = wide_nb(d, vec, ask)) {
        c.wide = nb;
        c.nt = nb;
        return c;
    }
    if (d->dtype == DS_DTYPE_BF16) {
        // staging-bound at 16x the matrix rate: the widest tile that does not pad Cout beyond the next 32
        c.bf16 = true;
        int best = 4, best_pad = 1 << 30;
        for (int nt = 4; nt >= 2; --nt) {
            const int pad = (N + 32 * nt - 1) / (32 * nt) * (32 * nt);
            if (pad < best_pad) { best_pad = pad; best = nt; }
        }
        c.nt = N <= 32 ? 1 : best;
        if (d->tile_nt > 0) c.nt = d->tile_nt > 4 ? 4 : d->tile_nt;
        if (t.nt > 0) c.nt = t.nt > 4 ? 4 : t.nt;
        return c;
    }
    // Measured on MI355X over every conv/GEMM shape of the joint step (profiles/r01_tile_sweep.txt):
    // latency-bound per wave, so small tiles at 3-5 resident workgroups per CU beat wide ones.
    const int64_t row_tiles = (M + 127) / 128;
    if (pad64 * 100 <= pad32 * 112 && row_tiles * (pad64 / 64) >= 5 * ds::kCUs / 2) c.nt = 2;
    if (d->tile_nt > 0) c.nt = d->tile_nt > 6 ? 6 : d->tile_nt;     // per-layer choice (tuning table)
    if (t.mt > 0) c.mt = t.mt;
    if (t.nt > 0) c.nt = t.nt;
    // LDS-DMA kernel (K-tile 32): needs 16-byte aligned operands and no folded stem.  Automatic for the
    // multi-tap convs whose reduction the 32-deep K-tile pads by no more than ~12 % over the 16-deep one:
    // measured 3-10 % faster there (long K loops), 5-10 % slower on the 1x1 layers whose 9-26 K-tiles
    // leave the prologue/epilogue exposed (profiles/r01_glds_sweep.txt).
    if (vec && d->fold_cin == 0 && t.path != 1) {
        const int k16 = (d->Cin + 15) / 16 * 16, k32 = (d->Cin + 31) / 32 * 32;
        if (t.path == 3 || (d->KH * d->KW >= 4 && k32 * 100 <= k16 * 112)) {
            c.glds = true;
            c.mt = 1;
            if (c.nt > 3) c.nt = 3;
        }
    }
    return c;
}

// Launch geometry (measured over every shape of the joint step, profiles/r01_grid_search.txt):
//   * up to kOneTilePerWg row tiles: one workgroup per tile, handed out by the hardware dispatcher as
//     slots free up.  A static stride over few tiles per workgroup quantises badly (98 row tiles on
//     96 workgroups = two rounds; 392 tiles on 256 = half the chip doing double work) and cost
//     20-45 % on the 14x14 and 7x7 maps.
//   * larger maps (conv2b/2c, stem: 6272 / 25088 row tiles): persistent workgroups, one resident wave,
//     striding over row tiles -- same speed within 2 %, and the BatchNorm statistics stay at a few
//     hundred partials per channel instead of one per row tile.
constexpr int kOneTilePerWg = 2048;

// The launch ds_conv_igemm makes of `d` with operand pointers that are (`aligned`) or are not 16-byte aligned
Launch choose(const ds_conv_desc *d, bool aligned, Ask ask = kAsIs) {
    Launch L;
    L.v = {d->w_n_stride == 1 && d->w_k_stride != 1, d->fold_cin > 0, dims_vec(d) && aligned};
    const TileCfg c = L.c = pick_cfg(d, L.v.vec, ask);
    L.bnr = false;          // (a DS_EPI_BN_RELU launch keeps the grid the descriptor gets without the flag)
    L.pool = d->pool_argmax || ask == kBeforePool;
    L.bnb = d->bnb != nullptr;
    const int bm = 128 * (c.glds ? 1 : c.mt), bn = 32 * c.nt;
    L.row_tiles = (int)((conv_M(d) + bm - 1) / bm);
    if (c.wide && L.pool) {          // 32-row blocks of whole image rows, four per workgroup
        int rpb, bpi;
        pool3_blocks(d, &rpb, &bpi);
        L.row_tiles = (int)(((int64_t)d->N * bpi + 3) / 4);
    }
    L.gy = (d->Cout + bn - 1) / bn;
    L.gx = L.row_tiles;
    L.one = true;
    // (the wide 1x1 kernel: always one workgroup per (row group, column tile))
    if (!c.wide && L.row_tiles > kOneTilePerWg) {
        int target = (resident_per_cu(kernel_of(L)) * ds::kCUs) / L.gy;             // one resident wave of workgroups
        if (target < 8) target = 8;
        L.gx = L.row_tiles < target ? L.row_tiles : target;
        if (L.gx >= 8) L.gx &= ~7;                  // multiple of 8: column tiles of a row tile share an XCD
        L.one = false;
    }
    if (d->grid_x > 0) {       // per-layer override
        L.gx = d->grid_x < L.row_tiles ? d->grid_x : L.row_tiles;
        L.one = L.gx == L.row_tiles;
    }
    L.bnr = (d->flags & DS_EPI_BN_RELU) != 0;
    L.grid = dim3(L.gx, L.gy, d->splits > 1 ? d->splits : 1);
    L.col_tiles = 0;
    if (L.one && (c.wide || (tuning().xcd_remap && L.gy > 1))) {    // one workgroup per tile: 1-D XCD-aware launch (TileId)
        L.col_tiles = L.gy;
        L.grid = dim3((L.row_tiles * L.gy + 7) / 8 * 8, 1, L.grid.z);
    }
    L.partials = L.gx;
    return L;
}

// Would the launch picked for `d` carry DS_EPI_BN_RELU?  The forward fp32 instantiations: n-contiguous weights, 16-byte loads
// (pointer alignment is checked at launch), 128-row tiles of the LDS / LDS-DMA kernels or the wide 1x1 kernel.
bool bnr_ok(const ds_conv_desc *d, const Launch &L) {
    if (d->dtype != DS_DTYPE_F32 || !L.v.bnmajor || !L.v.vec || L.v.fold || d->splits > 1 || d->bnb) return false;
    return !L.c.bf16 && L.c.mt == 1;
}

// What the four launchers of this file fill alike: the operands, M, the taps and the extents of the two buffer descriptors
// (bytes from the operand pointer to the last element read; `prepared_w_bytes` < 0: the strided filter `d` describes)
int fill_params(ConvParams &p, const char *who, const char *hint, const ds_conv_desc *d, const void *x, const void *w, float *z,
                const void *mask, float *stats, const float *pivot, int64_t prepared_w_bytes = -1) {
    p = ConvParams{};
    p.d = *d;
    if (d->splits <= 1) p.d.z_split_stride = 0;
    p.x = (const float *)x; p.w = (const float *)w; p.z = z; p.mask = (const float *)mask; p.stats = stats;
    p.pivot = (d->flags & DS_EPI_STATS) ? pivot : nullptr;
    p.M = (int)conv_M(d);
    p.taps = d->KH * d->KW;
    const int64_t x_elems = ((int64_t)d->N * d->H * d->W - 1) * d->ldx + (d->fold_cin > 0 ? d->fold_cin : d->Cin);
    const int64_t w_elems = (int64_t)(p.taps - 1) * d->w_tap_stride + (int64_t)(d->Cout - 1) * d->w_n_stride +
                            (int64_t)(d->Cin - 1) * d->w_k_stride + 1;
    const int64_t w_bytes = prepared_w_bytes < 0 ? w_elems * 4 : prepared_w_bytes;
    DS_REQUIRE(x_elems * 4 < (1ll << 31) && w_bytes < (1ll << 31), "%s: operand larger than 2 GiB%s", who, hint);
    p.x_bytes = (unsigned)(x_elems * 4);
    p.w_bytes = (unsigned)w_bytes;
    return DS_OK;
}

int igemm_launch(const ds_conv_desc *d, const float *x, const float *w, float *z, const float *bias, const float *mask,
                 float *stats, const float *pivot, const float *scale, const float *shift, void *stream) {
    DS_REQUIRE(d && x && w && z, "ds_conv_igemm: null argument");
    DS_REQUIRE(d->Cin > 0 && d->Cout > 0 && d->N > 0 && d->OH > 0 && d->OW > 0, "ds_conv_igemm: bad dims");
    DS_REQUIRE(d->w_n_stride == 1 || d->w_k_stride == 1, "ds_conv_igemm: one weight stride must be 1");
    DS_REQUIRE(!(d->flags & DS_EPI_BIAS) || bias, "ds_conv_igemm: DS_EPI_BIAS without bias");
    DS_REQUIRE(!(d->flags & DS_EPI_MASK) || mask, "ds_conv_igemm: DS_EPI_MASK without mask");
    DS_REQUIRE(!(d->flags & DS_EPI_STATS) || stats, "ds_conv_igemm: DS_EPI_STATS without stats buffer");
    DS_REQUIRE(!(d->flags & DS_EPI_BNSUMS) || (stats && mask && !(d->flags & (DS_EPI_STATS | DS_EPI_MASK)) && d->ldmask >= d->Cout),
               "ds_conv_igemm: DS_EPI_BNSUMS needs the partials buffer (stats), y (mask, ldmask) and excludes STATS / MASK");
    DS_REQUIRE(conv_M(d) < (1ll << 31), "ds_conv_igemm: M too large");
    DS_REQUIRE(d->dtype == DS_DTYPE_F32 || d->dtype == DS_DTYPE_BF16, "ds_conv_igemm: dtype must be DS_DTYPE_F32 or DS_DTYPE_BF16");
    const Launch L = choose(d, aligned16(x, w));
    const Variant &v = L.v;
    const TileCfg &c = L.c;
    DS_REQUIRE(!(d->flags & DS_EPI_STATS) || v.vec == dims_vec(d),
               "ds_conv_igemm: DS_EPI_STATS needs 16-byte aligned operand pointers");

    ConvParams p;
    if (int rc = fill_params(p, "ds_conv_igemm", " (split the batch)", d, x, w, z, mask, stats, pivot)) return rc;
    p.bias = bias;
    p.prio_mode = tuning().prio;
    DS_REQUIRE(!v.fold || (v.bnmajor && v.vec && d->KW == 1 && d->fold_cin % 4 == 0 && d->ldx == d->fold_cin),
               "ds_conv_igemm: fold_cin needs KW=1, n-contiguous 16-byte-aligned weights, ldx==fold_cin");

    DS_REQUIRE(d->dtype != DS_DTYPE_BF16 || (v.vec && d->splits <= 1),
               "ds_conv_igemm: DS_DTYPE_BF16 needs 16-byte aligned operands with channel counts / strides divisible by 4, no split-K");
    DS_REQUIRE(d->splits <= 1 || (d->flags == 0 && d->z_split_stride >= (int64_t)(conv_M(d) - 1) * d->ldz + d->Cout),
               "ds_conv_igemm: split-K needs flags == 0 and non-overlapping output slabs");
    DS_REQUIRE(!L.bnr || (d->flags == DS_EPI_BN_RELU && scale && shift && bnr_ok(d, L)),
               "ds_conv_igemm: DS_EPI_BN_RELU excludes every other epilogue flag, needs scale / shift and a forward fp32 launch "
               "with 16-byte aligned operands (ds_conv_plan_enable_bn_relu)");
    p.scale = scale; p.shift = shift;
    DS_REQUIRE((!d->norm_rstd && !d->norm_shift) || (c.wide && d->norm_rstd && d->norm_shift && d->Cin <= 1024),
               "ds_conv_igemm: norm_rstd / norm_shift are implemented by the wide 1x1 kernel only (ds_conv_igemm_norm_supported)");
    DS_REQUIRE((!d->mask_rstd && !d->mask_shift) || ((d->flags & DS_EPI_BNSUMS) && d->mask_rstd && d->mask_shift),
               "ds_conv_igemm: mask_rstd / mask_shift go with DS_EPI_BNSUMS");
    DS_REQUIRE(!(d->flags & DS_EPI_BNSUMS) || c.wide,
               "ds_conv_igemm: DS_EPI_BNSUMS is implemented by the wide 1x1 kernel only (ds_conv_igemm_bnsums_supported)");
    // the statistics partial count the caller planned with (ds_conv_igemm_partials at plan time) must be the one this
    // launch writes: the tile choice depends on debug switches / environment caches that may have changed since
    DS_REQUIRE(!(d->flags & (DS_EPI_STATS | DS_EPI_BNSUMS)) || d->partials <= 0 || d->partials == L.partials,
               "ds_conv_igemm: the launch would write %d statistics partials but the plan was made for %d "
               "(a ds_debug_conv_set_* switch changed after planning?)", L.partials, d->partials);
    p.row_tiles = L.row_tiles;
    p.col_tiles = L.col_tiles;
    if (d->bnb) {
        const ds_bn_bwd_on_load &b = *d->bnb;
        DS_REQUIRE(c.wide && !v.bnmajor && d->Cin <= 1024 && !d->norm_rstd,
                   "ds_conv_igemm: ds_conv_desc.bnb is implemented by the wide 1x1 kernel for k-contiguous weights only "
                   "(ds_conv_igemm_bnb_supported)");
        DS_REQUIRE(b.mean && b.rstd && b.shift && b.coef && b.nseg >= 1 && b.nseg <= 3 && b.c_end[b.nseg - 1] == d->Cin,
                   "ds_conv_igemm: bnb needs mean / rstd / shift / coef and 1..3 channel ranges that end at Cin");
        for (int i = 0; i < b.nseg; ++i) {
            const int cb = i ? b.c_end[i - 1] : 0;
            DS_REQUIRE(b.dy[i] && (((uintptr_t)b.dy[i]) & 15) == 0 && b.ld[i] % 4 == 0 && b.c_end[i] > cb && cb % 16 == 0 &&
                           b.ld[i] >= b.c_end[i] - cb && ((int64_t)(p.M - 1) * b.ld[i] + (b.c_end[i] - cb)) * 4 < (1ll << 31),
                       "ds_conv_igemm: bnb channel range %d (16-byte aligned dy, ld %% 4 == 0, boundaries %% 16 == 0)", i);
        }
        p.bnb = b;
    }
    if (d->pool_argmax) {
        DS_REQUIRE(c.wide && v.bnmajor && !d->bnb,
                   "ds_conv_igemm: ds_conv_desc.pool_argmax is implemented by the wide 1x1 kernel's forward instantiation only "
                   "(ds_conv_igemm_pool3_supported)");
        pool3_blocks(d, &p.pool_rpb, &p.pool_bpi);
    }
    hipLaunchKernelGGL(kernel_of(L), L.grid, dim3(256), 0, (hipStream_t)stream, p);
    return ds::check_launch("ds_conv_igemm");
}

}  // namespace

#ifdef DS_TUNING
extern "C" int ds_debug_conv_set_tile(int mt, int nt) {
    DS_REQUIRE((mt == 0 && nt == 0) || ((mt == 1 || mt == 2) && nt >= 1 && nt <= 6), "ds_debug_conv_set_tile: mt in {1,2}, nt in 1..6, or 0,0 = automatic");
    tuning().mt = mt;
    tuning().nt = nt;
    return DS_OK;
}

extern "C" int ds_debug_conv_set_wide(int mode) {
    DS_REQUIRE(mode >= 0 && mode <= 2, "ds_debug_conv_set_wide: 0 = never, 1 = automatic, 2 = wherever the shape allows");
    tuning().wide = mode;
    return DS_OK;
}

extern "C" int ds_debug_conv_set_wide_nb(int nb) {
    DS_REQUIRE(nb >= 0 && nb <= 8, "ds_debug_conv_set_wide_nb: 0 = the cost model, 1 .. 8 column blocks per wave");
    tuning().wide_nb = nb;          // (wide_nb: a pin above the launch's own cap is ignored; POOL keeps ceil(Cout / 32))
    return DS_OK;
}

extern "C" int ds_debug_conv_igemm_launch(const ds_conv_desc *d, int out[10]) {
    DS_REQUIRE(d && out, "ds_debug_conv_igemm_launch: null argument");
    const Launch L = choose(d, true);
    out[0] = L.c.wide;
    out[1] = L.v.bnmajor ? 1 : 0;
    out[2] = L.bnb ? 1 : 0;
    out[3] = L.pool ? 1 : 0;
    out[4] = L.bnr ? 1 : 0;
    out[5] = L.c.mt;
    out[6] = L.c.nt;
    out[7] = L.c.glds ? 1 : 0;
    out[8] = (int)(L.grid.x * L.grid.y * L.grid.z);
    out[9] = L.partials;
    return DS_OK;
}

extern "C" int ds_debug_conv_set_path(int path) {
    DS_REQUIRE(path == 0 || path == 1 || path == 3,
               "ds_debug_conv_set_path: 0 = automatic, 1 = register-staged LDS kernel, 3 = LDS-DMA kernel (2, the register-direct kernel, is retired)");
    tuning().path = path;
    return DS_OK;
}

extern "C" int ds_debug_conv_bf16_set_max_nb(int nb) {
    DS_REQUIRE(nb >= 1 && nb <= 8, "ds_debug_conv_bf16_set_max_nb: 1 .. 8 column blocks per wave");
    tuning().bf16d_max_nb = nb;
    return 0;
}
#endif

// ---- plan-time questions: each is asked of the launch choose() makes, with 16-byte aligned operands assumed (BatchNorm convs
// are always aligned in this model; ds_conv_igemm refuses DS_EPI_STATS when the operands turn out not to be, so the count
// returned here is the one the launch uses)
extern "C" int ds_conv_igemm_partials(const ds_conv_desc *d) { return choose(d, true).partials; }

extern "C" int ds_conv_igemm_bnsums_supported(const ds_conv_desc *d) {
    // DS_EPI_BNSUMS lives in the wide 1x1 kernel's epilogue: supported where that kernel is the one chosen
    if (!d) return 0;
    ds_conv_desc t = *d;
    t.flags = (t.flags & DS_EPI_ACCUM) | DS_EPI_BNSUMS;
    return choose(&t, true).c.wide > 0 ? 1 : 0;
}

extern "C" int ds_conv_igemm_norm_supported(const ds_conv_desc *d) {
    // BatchNorm + ReLU on load lives in the wide 1x1 kernel's loader (Cin <= 1024: the per-channel values sit in LDS)
    if (!d || d->Cin > 1024) return 0;
    return choose(d, true).c.wide > 0 ? 1 : 0;
}

extern "C" int ds_conv_igemm_pool3_supported(const ds_conv_desc *d) {
    // the 3x3 / 1 max pool on load lives in the wide 1x1 kernel's loader (forward instantiation)
    if (!d) return 0;
    return choose(d, true, kBeforePool).c.wide > 0 ? 1 : 0;
}

// ds_conv_plan_enable_bn_relu's question for this family: would the launch picked for `d` carry DS_EPI_BN_RELU?  (forward
// fp32: n-contiguous weights, strides and channel counts divisible by 4, LDS-tile / LDS-DMA / wide 1x1 kernel, with or
// without pool_argmax; the kernel and tile are the ones the same descriptor gets without the flag)
namespace ds {
int conv_igemm_bn_relu_supported(const ds_conv_desc *d) {
    if (!d || (d->flags & ~DS_EPI_BN_RELU)) return 0;
    ds_conv_desc t = *d;
    t.flags = DS_EPI_BN_RELU;
    return bnr_ok(&t, choose(&t, true)) ? 1 : 0;
}
}  // namespace ds

extern "C" int ds_conv_igemm_bnb_supported(const ds_conv_desc *d) {
    // BatchNorm backward on load lives in the wide 1x1 kernel's loader, k-contiguous-weights (dgrad) instantiation
    if (!d || d->Cin > 1024 || (d->w_n_stride == 1 && d->w_k_stride != 1) || d->norm_rstd) return 0;
    return choose(d, true, kBeforeBnb).c.wide > 0 ? 1 : 0;      // with the launch's own cap of two column blocks per wave
}

extern "C" int ds_conv_igemm(const ds_conv_desc *d, const float *x, const float *w, float *z, const float *bias,
                             const float *mask, float *stats, const float *pivot, void *stream) {
    DS_REQUIRE(!d || !(d->flags & DS_EPI_BN_RELU), "ds_conv_igemm: DS_EPI_BN_RELU takes its scale / shift through ds_conv_run (ds_conv_io)");
    return igemm_launch(d, x, w, z, bias, mask, stats, pivot, nullptr, nullptr, stream);
}

// ds_conv_run's entry for DS_EPI_BN_RELU plans of this family
namespace ds {
int conv_igemm_bn_relu(const ds_conv_desc *d, const float *x, const float *w, float *z, const float *scale, const float *shift,
                       void *stream) {
    DS_REQUIRE(d && (d->flags & DS_EPI_BN_RELU) && scale && shift, "ds_conv_run: DS_EPI_BN_RELU without scale / shift");
    return igemm_launch(d, x, w, z, nullptr, nullptr, nullptr, nullptr, scale, shift, stream);
}
}  // namespace ds

// One launch for `count` (1..4) independent GEMMs, each described as for ds_conv_igemm (split-K descriptors write their slabs
// at z[i] + s * z_split_stride).  Problem i's tiles receive exactly what ds_conv_igemm(descs[i], x[i], w[i], z[i]) writes: the
// grid of that launch (choose) is laid into this one and the workgroups run the same code.  Plain 1x1 fp32 problems without
// epilogue whose own launch is the 128 x 32 LDS-staged tile (the batch x features GEMMs of the heads); anything else is DS_ERR_ARG.
extern "C" int ds_gemm_group(const ds_conv_desc *const *descs, const float *const *x, const float *const *w, float *const *z,
                             int32_t count, void *stream) {
    DS_REQUIRE(descs && x && w && z && count >= 1 && count <= kGemmGroupMax, "ds_gemm_group: 1..%d problems", kGemmGroupMax);
    GemmGroupParams g{};
    g.count = count;
    int wgs = 0;
    for (int i = 0; i < count; ++i) {
        const ds_conv_desc *d = descs[i];
        DS_REQUIRE(d && x[i] && w[i] && z[i], "ds_gemm_group: null argument (problem %d)", i);
        DS_REQUIRE(d->Cin > 0 && d->Cout > 0 && d->N > 0 && d->KH == 1 && d->KW == 1 && d->stride == 1 && d->H == 1 && d->W == 1 &&
                       d->OH == 1 && d->OW == 1 && d->pad_t == 0 && d->pad_l == 0 && d->fold_cin == 0 && d->flip == 0,
                   "ds_gemm_group: problem %d is not a plain GEMM", i);
        DS_REQUIRE(d->dtype == DS_DTYPE_F32 && d->flags == 0 && !d->bnb && !d->norm_rstd && !d->norm_shift &&
                       !d->mask_rstd && !d->mask_shift && !d->pool_argmax,
                   "ds_gemm_group: problem %d: fp32 without epilogue flags or on-load operands (combine with ds_slab_epilogue_group)", i);
        DS_REQUIRE(d->w_n_stride == 1 || d->w_k_stride == 1, "ds_gemm_group: one weight stride must be 1");
        DS_REQUIRE(d->ldx >= d->Cin && d->ldz >= d->Cout, "ds_gemm_group: problem %d: row strides below the row lengths", i);
        DS_REQUIRE(d->splits <= 1 || d->z_split_stride >= (int64_t)(d->N - 1) * d->ldz + d->Cout,
                   "ds_gemm_group: problem %d: overlapping output slabs", i);
        const Launch L = choose(d, aligned16(x[i], w[i]));
        const TileCfg &c = L.c;
        DS_REQUIRE(c.mt == 1 && c.nt == 1 && !c.glds && !c.bf16 && !c.wide,
                   "ds_gemm_group: problem %d's own launch is not the 128 x 32 tile (run it through ds_conv_igemm)", i);
        ConvParams &p = g.p[i];
        if (int rc = fill_params(p, "ds_gemm_group", "", d, x[i], w[i], z[i], nullptr, nullptr, nullptr)) return rc;
        p.row_tiles = L.row_tiles;
        p.col_tiles = L.col_tiles;
        g.gx[i] = L.grid.x; g.gy[i] = L.grid.y; g.splits[i] = L.grid.z;
        g.variant[i] = (L.v.bnmajor ? 1 : 0) | (L.v.vec ? 2 : 0);
        const int64_t own = (int64_t)L.grid.x * L.grid.y * L.grid.z;
        DS_REQUIRE(wgs + own < (1 << 20), "ds_gemm_group: too many workgroups");
        wgs += (int)own;
        g.wg_end[i] = wgs;
    }
    hipLaunchKernelGGL(gemm_group_kernel, dim3(wgs), dim3(256), 0, (hipStream_t)stream, g);
    return ds::check_launch("ds_gemm_group");
}

// ---- bf16 register-direct path -------------------------------------------------------------------------------------
namespace {
int bf16d_nb(int Cout, bool x16_1x1) {
    // a workgroup's cost per K step ~ (A fetch + NB MFMAs); minimise column tiles x (c + NB), c ~ 4, ties to wider.
    // 1x1 launches from 16-bit activation storage are pure streaming (8 passes per 16 channels): at most four column blocks
    // per wave, i.e. 3-4 waves per SIMD instead of 2 -- twelve 1x1 shapes of the tower, forward with statistics:
    // 479 -> 434 us (scripts/bf16_wide_sweep.py); the input gradients (fp32 dz) keep eight (492 against 521)
    const int max_nb = tuning().bf16d_max_nb;
    const int top = x16_1x1 && max_nb > 4 ? 4 : max_nb;
    int best = top, best_cost = 1 << 30;
    for (int nb = top; nb >= 1; --nb) {
        const int tiles = (Cout + 32 * nb - 1) / (32 * nb);
        const int cost = tiles * (4 + nb);
        if (cost < best_cost) { best_cost = cost; best = nb; }
    }
    return best;
}
bool bf16d_ok(const ds_conv_desc *d) {
    return (d->KH == d->KW) && (d->KH == 1 || d->KH == 3) && d->fold_cin == 0 && d->Cin % 8 == 0 && d->ldx % 4 == 0 &&
           !(d->flags & ~(DS_EPI_STATS | DS_EPI_ACCUM | DS_EPI_BNSUMS)) &&
           !((d->flags & DS_EPI_BNSUMS) && (d->flags & DS_EPI_STATS)) && d->splits <= 1 &&
           // the epilogue addresses z (and the BatchNorm-sums activation) through 32-bit buffer offsets
           ((conv_M(d) - 1) * d->ldz + d->Cout) * 4 < (1ll << 31) &&
           (!(d->flags & DS_EPI_BNSUMS) || ((conv_M(d) - 1) * d->ldmask + d->Cout) * 4 < (1ll << 31));
}

// The launch ds_conv_bf16 and ds_conv_f32x3 share: conv_bf16d_kernel<NB = nb, ..> on the prepared weights (`planes` bf16 planes),
// 128 rows x 32 * nb columns per workgroup, on the 1-D XCD-aware grid (TileId)
int bf16d_launch(const char *who, const ds_conv_desc *d, const void *x, const void *wb, int planes, float *z, const void *mask,
                 float *stats, const float *pivot, int nb, KernelFn kernel, void *stream) {
    ConvParams p;
    const int64_t wb_bytes = planes * (int64_t)((d->Cin + 15) / 16) * (d->KH * d->KW) * ((d->Cout + 31) / 32 * 32) * 32;
    if (int rc = fill_params(p, who, "", d, x, wb, z, mask, stats, pivot, wb_bytes)) return rc;
    if (d->x_dtype == DS_DTYPE_BF16) p.x_bytes /= 2;
    p.col_total = (d->Cout + 31) / 32 * 32;
    p.row_tiles = (int)((conv_M(d) + 127) / 128);
    p.col_tiles = (d->Cout + 32 * nb - 1) / (32 * nb);
    const dim3 grid((unsigned)(((int64_t)p.row_tiles * p.col_tiles + 7) / 8 * 8));
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, (hipStream_t)stream, p);
    return ds::check_launch(who);
}
}  // namespace

extern "C" size_t ds_weights_bf16_bytes(int32_t Cin, int32_t Cout, int32_t taps, int32_t dgrad) {
    const int K = dgrad ? Cout : Cin, Ncol = dgrad ? Cin : Cout;
    return (size_t)((K + 15) / 16) * taps * ((Ncol + 31) / 32 * 32) * 16 * 2;
}

extern "C" int ds_weights_to_bf16(const float *w, void *wb, int32_t Cin, int32_t Cout, int32_t taps, int32_t dgrad,
                                  void *stream) {
    DS_REQUIRE(w && wb && Cin > 0 && Cout > 0 && taps > 0, "ds_weights_to_bf16: bad argument");
    const int64_t total = (int64_t)ds_weights_bf16_bytes(Cin, Cout, taps, dgrad) / 2;
    hipLaunchKernelGGL(weights_to_bf16_kernel, dim3(ds::stream_grid(total, 256)), dim3(256), 0, (hipStream_t)stream, w,
                       (__bf16 *)wb, Cin, Cout, taps, dgrad);
    return ds::check_launch("ds_weights_to_bf16");
}

extern "C" int ds_conv_bf16_supported(const ds_conv_desc *d) { return d && bf16d_ok(d) ? 1 : 0; }

extern "C" int ds_conv_bf16_partials(const ds_conv_desc *d) { return (int)((conv_M(d) + 127) / 128); }

extern "C" int ds_conv_bf16(const ds_conv_desc *d, const void *x, const void *wb, float *z, const void *mask, float *stats,
                            const float *pivot, void *stream) {
    DS_REQUIRE(d && x && wb && z, "ds_conv_bf16: null argument");
    DS_REQUIRE(!(d->flags & DS_EPI_BNSUMS) || (mask && stats && d->ldmask >= d->Cout &&
                                               (d->mask_dtype == DS_DTYPE_F32 || d->mask_dtype == DS_DTYPE_BF16)),
               "ds_conv_bf16: DS_EPI_BNSUMS needs mask (row stride ldmask, mask_dtype) and a partials buffer");
    DS_REQUIRE(!d->mask_rstd && !d->norm_rstd && !d->bnb, "ds_conv_bf16: the on-load transforms belong to the fp32 kernels");
    DS_REQUIRE(d->x_dtype == DS_DTYPE_F32 || (d->x_dtype == DS_DTYPE_BF16 && d->ldx % 8 == 0),
               "ds_conv_bf16: x_dtype must be DS_DTYPE_F32 or DS_DTYPE_BF16 (then ldx %% 8 == 0)");
    const bool xb = d->x_dtype == DS_DTYPE_BF16;
    DS_REQUIRE(bf16d_ok(d), "ds_conv_bf16: needs a 1x1 or 3x3 conv, Cin %% 8 == 0, ldx %% 4 == 0, flags within DS_EPI_STATS, or "
                            "DS_EPI_ACCUM | DS_EPI_BNSUMS for a dgrad");
    DS_REQUIRE(aligned16(x, wb) && conv_M(d) < (1ll << 31), "ds_conv_bf16: operands must be 16-byte aligned");
    DS_REQUIRE(!(d->flags & DS_EPI_STATS) || stats, "ds_conv_bf16: DS_EPI_STATS without stats buffer");
    DS_REQUIRE(d->z_dtype == DS_DTYPE_F32 || (d->z_dtype == DS_DTYPE_BF16 && !(d->flags & (DS_EPI_ACCUM | DS_EPI_BNSUMS))),
               "ds_conv_bf16: the output in bf16 storage excludes the accumulate / BatchNorm-sums epilogues");
    const int nb = bf16d_nb(d->Cout, xb && d->KH == 1);
    const KernelFn kernel = with_const<1, 8>(nb, [&](auto n) {
        constexpr int NB = decltype(n)::value;
        if (xb) return d->KH == 1 ? conv_bf16d_kernel<NB, 1, true> : conv_bf16d_kernel<NB, 3, true>;
        return d->KH == 1 ? conv_bf16d_kernel<NB, 1, false> : conv_bf16d_kernel<NB, 3, false>;
    });
    return bf16d_launch("ds_conv_bf16", d, x, wb, 1, z, mask, stats, pivot, nb, kernel, stream);
}

// ---- fp32 products on the bf16 matrix cores (see conv_bf16d_kernel<.., X3>) ----------------------------------------
extern "C" size_t ds_weights_f32x3_bytes(int32_t Cin, int32_t Cout, int32_t taps, int32_t dgrad) {
    return 3 * ds_weights_bf16_bytes(Cin, Cout, taps, dgrad);
}

extern "C" int ds_weights_to_f32x3(const float *w, void *wb, int32_t Cin, int32_t Cout, int32_t taps, int32_t dgrad,
                                   void *stream) {
    DS_REQUIRE(w && wb && Cin > 0 && Cout > 0 && taps > 0, "ds_weights_to_f32x3: bad argument");
    const int64_t total = (int64_t)ds_weights_bf16_bytes(Cin, Cout, taps, dgrad) / 2;
    hipLaunchKernelGGL(weights_to_f32x3_kernel, dim3(ds::stream_grid(total, 256)), dim3(256), 0, (hipStream_t)stream, w,
                       (__bf16 *)wb, Cin, Cout, taps, dgrad);
    return ds::check_launch("ds_weights_to_f32x3");
}

extern "C" int ds_conv_f32x3_supported(const ds_conv_desc *d) {
    if (!d) return 0;
    ds_conv_desc t = *d;
    t.flags &= ~(DS_EPI_ACCUM | DS_EPI_BNSUMS);             // (the X3 epilogue also accumulates and emits BatchNorm sums)
    if ((d->flags & DS_EPI_BNSUMS) && (d->flags & DS_EPI_STATS)) return 0;
    return bf16d_ok(&t) && d->x_dtype == DS_DTYPE_F32 && (!d->norm_rstd || (d->KH == 1 && d->Cin <= 1024)) ? 1 : 0;
}

extern "C" int ds_conv_f32x3_partials(const ds_conv_desc *d) { return (int)((conv_M(d) + 127) / 128); }

extern "C" int ds_conv_f32x3(const ds_conv_desc *d, const float *x, const void *wb, float *z, const float *mask,
                             float *stats, const float *pivot, void *stream) {
    DS_REQUIRE(d && x && wb && z, "ds_conv_f32x3: null argument");
    DS_REQUIRE(ds_conv_f32x3_supported(d),
               "ds_conv_f32x3: needs a 1x1 or 3x3 conv on fp32 x, Cin %% 8 == 0, ldx %% 4 == 0, flags within DS_EPI_STATS | "
               "DS_EPI_ACCUM | DS_EPI_BNSUMS (norm_rstd / norm_shift: 1x1 only, Cin <= 1024)");
    DS_REQUIRE((!d->norm_rstd) == (!d->norm_shift) && (!d->mask_rstd) == (!d->mask_shift) &&
                   (!d->mask_rstd || (d->flags & DS_EPI_BNSUMS)),
               "ds_conv_f32x3: norm_rstd / norm_shift and mask_rstd / mask_shift come in pairs (the latter with DS_EPI_BNSUMS)");
    DS_REQUIRE(!(d->flags & DS_EPI_BNSUMS) || (mask && stats && d->ldmask >= d->Cout),
               "ds_conv_f32x3: DS_EPI_BNSUMS needs mask (row stride ldmask) and a partials buffer");
    DS_REQUIRE(aligned16(x, wb) && conv_M(d) < (1ll << 31), "ds_conv_f32x3: operands must be 16-byte aligned");
    DS_REQUIRE(!(d->flags & DS_EPI_STATS) || stats, "ds_conv_f32x3: DS_EPI_STATS without stats buffer");
    // two column blocks per wave (one where Cout <= 32): measured best on all fourteen 1x1 layer shapes (NB = 4: the
    // split is better amortised but two waves per SIMD no longer fit; profiles/r03_f32x3_layers.txt)
    const int nb = d->Cout <= 32 ? 1 : 2;
    const KernelFn kernel = with_const<1, 2>(nb, [&](auto n) {
        return d->KH == 1 ? conv_bf16d_kernel<decltype(n)::value, 1, false, true> : conv_bf16d_kernel<decltype(n)::value, 3, false, true>;
    });
    return bf16d_launch("ds_conv_f32x3", d, x, wb, 3, z, mask, stats, pivot, nb, kernel, stream);
}

