// 3x3 stride-1 SAME convolution (forward and dgrad) as fused Winograd F(2x2, 3x3) on the fp32 matrix cores.
//
// The 3x3 layers are 2/3 of Inception-v1's multiplies (image_model/inception_v1.py: Conv2d_2c_3x3 :74-75 and the
// Branch_1 / Branch_2 Conv2d_0b_3x3 of all nine Mixed blocks :86-247) and fp32 MFMA runs at the fp32 vector rate, so
// the direct implicit GEMM is bound by the matrix pipe even when everything else is hidden.  Winograd's minimal
// filtering trades 36 multiplies per 2x2 output tile and channel pair for 16:
//     Y = A^T [ (G g G^T) (.) (B^T d B) ] A            (Lavin & Gray, F(2x2, 3x3); cross-correlation form)
// i.e. sixteen independent GEMMs  M_xi[tile, co] = sum_ci V_xi[tile, ci] U_xi[ci, co]  over the sixteen positions
// xi of the transformed 4x4 patch -- 2.25x fewer MFMA passes for the same convolution.
//
// Fused form (nothing but x, the pre-transformed weights U and z touches memory):
//   * a wave owns 32 output tiles x 32 output channels and ALL sixteen positions: sixteen 32x32 fp32 accumulators
//     = 256 accumulator registers (gfx950's unified 512-register file at one wave per SIMD);
//   * lane (i, kh) of the 32x32x2 MFMA's A operand is tile i and channels 4 kh .. 4 kh + 3 of the 8-channel K step:
//     the lane loads the 16 pixels of its own 4x4 input patch as float4 (SRD loads, padding pixels and tiles past
//     the end read zeros from an out-of-range offset), runs B^T d B on them in registers (32 adds per channel) and
//     the sixteen results ARE its A fragments -- no LDS round trip, no im2col, no transformed-input tensor;
//   * the transformed weights U [16][Cout][Cin] (ci contiguous; made once per weight update by
//     ds_wino_transform_weights) are the B operand: the workgroup's [16][32][8] slice of a K step goes global -> LDS
//     by LDS-DMA (lane-linear = exactly this layout), double buffered, shared by the four waves (four different
//     32-tile groups, same 32 channels);
//   * the matrix pipe needs 64 cycles per MFMA, so between two MFMAs the wave has issue slots for the next
//     position's ds_read_b128 and for the loads of the next K step: per K step 64 MFMAs (4096 cycles) against
//     ~128 transform adds, 16 + 4 loads, 16 LDS reads and one barrier;
//   * epilogue: A^T M A per lane across the sixteen accumulators (the C layout is position independent), 2x2
//     outputs stored as 128-byte channel runs, BatchNorm column statistics about the pivot as in conv_igemm.hip.
// dgrad of a 3x3 stride-1 SAME conv is the same correlation over dz with the taps flipped and the channel roles
// swapped, so it is this kernel with U built from the flipped, transposed filter.
// Numerics: fp32 throughout; the transforms add ~1e-7-level rounding of their own (inputs are combined before the
// multiply), so results match the direct kernels to ~1e-6 relative, not bit for bit; reductions are ordered and
// deterministic.
#include <stdlib.h>
#include "conv_epilogue.h"

using ds::f32x16;
typedef float f32x4 __attribute__((ext_vector_type(4)));

namespace {

using ds::kOOB;
using ds::make_srd;

struct WinoParams {
    const float *x;         // [N, H, W, ldx]
    const float *u;         // [16][Cout][Cin]
    float *z;               // [N, H, W, ldz]
    float *stats;           // [2][Cout][P], P = groups
    const float *pivot;
    const float *y;         // DS_EPI_BNSUMS: forward activation of the layer that consumes z (= dy), same pixel stride ldz
    int N, H, W, Cin, ldx, Cout, ldz;
    int TH, TW, Mt;         // output tiles per column / row / in total
    int groups, ncol;       // 128-tile groups, 32-channel blocks
    unsigned x_bytes, u_bytes, z_bytes;
    int flags;
    const float *scale, *shift;      // DS_EPI_BN_RELU (conv_wino_kernel<false, true>): Cout floats each
};


typedef __attribute__((address_space(3))) void *lds_ptr;

// a - b on four floats as two v_pk_add_f32 with the second operand negated.  hipcc packs fp32 adds into
// v_pk_add_f32 by itself but leaves subtractions as four v_sub_f32, and with one wave per SIMD every VALU issue
// slot of the transform is a slot the matrix pipe idles (scripts/microbench/mfma_mix.hip: 64 MFMAs alone 1.73 us, with the K
// step's 128 VALU ops, 16 LDS reads and barrier 2.15 us): 112 -> 64 VALU instructions per K step, -4 % kernel time.
typedef float f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f32x4 sub4(f32x4 a, f32x4 b) {
    f32x2 lo, hi;
    const f32x2 alo = {a[0], a[1]}, ahi = {a[2], a[3]}, blo = {b[0], b[1]}, bhi = {b[2], b[3]};
    asm("v_pk_add_f32 %0, %1, %2 neg_lo:[0,1] neg_hi:[0,1]" : "=v"(lo) : "v"(alo), "v"(blo));
    asm("v_pk_add_f32 %0, %1, %2 neg_lo:[0,1] neg_hi:[0,1]" : "=v"(hi) : "v"(ahi), "v"(bhi));
    return f32x4{lo[0], lo[1], hi[0], hi[1]};
}

// BNS: DS_EPI_BNSUMS epilogue (its own instantiation: the plain kernel's code is untouched); BNR: the inference epilogue
// DS_EPI_BN_RELU, y = max(fma(y, scale[col], shift[col]), 0) stored in place of z, no statistics (its own instantiation too)
template <bool BNS, bool BNR = false>
__global__ __launch_bounds__(256, 1) void conv_wino_kernel(const WinoParams p) {
    // B tile of one K step: [16 positions][32 channels][8 ci] floats = 16 KB, two buffers
    __shared__ __attribute__((aligned(128))) float smem[2 * 16 * 32 * 8];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 31, kh = lane >> 5;
    // 1-D XCD-aware launch (as conv_igemm.hip's TileId): the row-major list of (tile group, channel block) pairs is
    // cut into 8 contiguous ranges, one per XCD (workgroup id % 8, observed placement; a different one only costs
    // speed), so the channel blocks of a tile group -- which read the same input patches -- run back to back on one
    // XCD and the patches cross the fabric once per tile group instead of once per channel block.
    const int id = blockIdx.x;
    const int lin = (id & 7) * (int)(gridDim.x >> 3) + (id >> 3);
    const int group = lin / p.ncol, cblk = lin - group * p.ncol;
    const int co0 = cblk * 32;
    const int tile0 = group < p.groups ? (group * 4 + wave) * 32 : p.Mt;      // surplus workgroups own no tile
    const __amdgpu_buffer_rsrc_t srd_x = make_srd(p.x, p.x_bytes);
    const __amdgpu_buffer_rsrc_t srd_u = make_srd(p.u, p.u_bytes);

    // ---- this lane's tile: byte offsets of the 16 pixels of its 4x4 input patch (channel 4 kh) -------------
    const int m = tile0 + li;
    const bool tv = m < p.Mt;
    const int tpi = p.TH * p.TW;
    const int n = (tv ? m : 0) / tpi;
    const int r = (tv ? m : 0) - n * tpi;
    const int th = r / p.TW, tw = r - th * p.TW;
    unsigned voff[16];
#pragma unroll
    for (int py = 0; py < 4; ++py)
#pragma unroll
        for (int px = 0; px < 4; ++px) {
            const int ih = 2 * th - 1 + py, iw = 2 * tw - 1 + px;
            const bool ok = tv && (unsigned)ih < (unsigned)p.H && (unsigned)iw < (unsigned)p.W;
            voff[py * 4 + px] = ok ? (unsigned)(((n * p.H + ih) * p.W + iw) * p.ldx + 4 * kh) * 4u : kOOB;
        }
    // ---- B tile DMA slots: instruction i of wave w fills floats [(i*256 + w*64 + lane) * 4, +4) of the buffer ---
    unsigned uoff[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int idx = i * 256 + tid;                  // (xi, co, half) = (idx / 64, (idx / 2) % 32, idx % 2)
        const int xi = idx >> 6, co = (idx >> 1) & 31, half = idx & 1;
        uoff[i] = (co0 + co < p.Cout) ? (unsigned)(((xi * p.Cout + co0 + co) * p.Cin) + 4 * half) * 4u : kOOB;
    }

    f32x16 acc[16];
#pragma unroll
    for (int xi = 0; xi < 16; ++xi)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[xi][e] = 0.f;

    f32x4 raw[16];
    auto load_raw = [&](int c0) {
#pragma unroll
        for (int q = 0; q < 16; ++q)
            raw[q] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(srd_x, voff[q], c0 * 4, 0));
    };
    auto dma_u = [&](int buf, int c0) {
        float *dst = smem + buf * 4096 + wave * 256;
#pragma unroll
        for (int i = 0; i < 4; ++i)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(srd_u, (lds_ptr)(dst + i * 1024), 16, uoff[i], c0 * 4, 0, 0);
    };

    const int ksteps = p.Cin >> 3;
    load_raw(0);
    dma_u(0, 0);
    __syncthreads();
    for (int ks = 0; ks < ksteps; ++ks) {
        // ---- V = B^T d B on the 16 pixels, per channel component: the results are the A fragments.  The row pass
        // (B^T d) needs all 16 pixels and runs first; the column pass of patch row py+1 is issued behind the MFMAs of
        // row py, in the shadow of the last of them ----------------------------------------------------------------------
        f32x4 t[16];
#pragma unroll
        for (int px = 0; px < 4; ++px) {
            const f32x4 d0 = raw[px], d1 = raw[4 + px], d2 = raw[8 + px], d3 = raw[12 + px];
            t[px] = sub4(d0, d2);
            t[4 + px] = d1 + d2;
            t[8 + px] = sub4(d2, d1);
            t[12 + px] = sub4(d1, d3);
        }
        // Operands of the next K step are requested BETWEEN the MFMA groups, four patch pixels and one weight DMA per
        // patch row: each pixel-scattered load occupies the texture-address path for a while, and issued in one burst at
        // the top of the step they stall the wave's in-order issue with the matrix pipe idle (measured +0.8 us per
        // step); spread out, they sit in the shadow of the MFMAs in front of them.
        const bool more = ks + 1 < ksteps;
        const int cn = (ks + 1) * 8;
        float *dma_dst = smem + ((ks + 1) & 1) * 4096 + wave * 256;
        const float *b_s = smem + (ks & 1) * 4096 + li * 8 + kh * 4;
        f32x4 v[4], vn[4], b[4], bn[4];
        vn[0] = sub4(t[0], t[2]); vn[1] = t[1] + t[2]; vn[2] = sub4(t[2], t[1]); vn[3] = sub4(t[1], t[3]);
#pragma unroll
        for (int px = 0; px < 4; ++px) bn[px] = *reinterpret_cast<const f32x4 *>(b_s + px * 256);
#pragma unroll
        for (int py = 0; py < 4; ++py) {
#pragma unroll
            for (int j = 0; j < 4; ++j) { v[j] = vn[j]; b[j] = bn[j]; }
            if (py < 3) {       // the next row's weights are read while this row's sixteen MFMAs run
#pragma unroll
                for (int px = 0; px < 4; ++px) bn[px] = *reinterpret_cast<const f32x4 *>(b_s + (py * 4 + 4 + px) * 256);
            }
            if (more) {
                // (flags 256 / 512 / 1024 switch the pixel loads / weight DMAs / stores off for timing experiments.  The
                // uniform branches also keep hipcc from regrouping the requests: with them removed the same kernel
                // measured 5.7 % slower, with the loads made unconditional 2 % slower -- scratch A/B on one box.)
                if (!(p.flags & 256)) {
#pragma unroll
                    for (int px = 0; px < 4; ++px)
                        raw[py * 4 + px] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(srd_x, voff[py * 4 + px], cn * 4, 0));
                }
                if (!(p.flags & 512))
                    __builtin_amdgcn_raw_ptr_buffer_load_lds(srd_u, (lds_ptr)(dma_dst + py * 1024), 16, uoff[py], cn * 4, 0, 0);
            }
            __builtin_amdgcn_sched_barrier(0);
            // positions of this patch row, two at a time: consecutive MFMAs alternate between two accumulators
#pragma unroll
            for (int pp = 0; pp < 4; pp += 2)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    acc[py * 4 + pp] = __builtin_amdgcn_mfma_f32_32x32x2f32(v[pp][j], b[pp][j], acc[py * 4 + pp], 0, 0, 0);
                    acc[py * 4 + pp + 1] = __builtin_amdgcn_mfma_f32_32x32x2f32(v[pp + 1][j], b[pp + 1][j], acc[py * 4 + pp + 1], 0, 0, 0);
                }
            if (py < 3) {       // column pass of the next patch row, behind this row's MFMAs
                const f32x4 t0 = t[py * 4 + 4], t1 = t[py * 4 + 5], t2 = t[py * 4 + 6], t3 = t[py * 4 + 7];
                vn[0] = sub4(t0, t2); vn[1] = t1 + t2; vn[2] = sub4(t2, t1); vn[3] = sub4(t1, t3);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        __syncthreads();
    }

    // ---- output transform Y = A^T M A, per lane across the sixteen accumulators; store; statistics ---------------
    // accumulator element e of every position is the same (tile row, channel column): row = (e&3) + 8 (e>>2) + 4 kh
    const int col = co0 + li;
    const bool colok = col < p.Cout;
    const float pv = (p.pivot && colok) ? p.pivot[col] : 0.f;
    const __amdgpu_buffer_rsrc_t srd_z = make_srd(p.z, p.z_bytes);
    // byte offset of the tile's top-left output pixel (channel 0), or out of range; bit 0 / 1 = the tile has a
    // right column / a bottom row inside the image (odd H, W).  Read from the lane that owns the tile with
    // v_readlane (the row of an accumulator element is a compile-time constant plus 4 kh).
    const unsigned obase = tv ? (unsigned)(((n * p.H + 2 * th) * p.W + 2 * tw) * p.ldz) * 4u : kOOB;
    const int oflags = tv ? ((2 * tw + 1 < p.W ? 1 : 0) | (2 * th + 1 < p.H ? 2 : 0)) : 0;
    const unsigned right = (unsigned)p.ldz * 4u, below = (unsigned)(p.W * p.ldz) * 4u;
    const unsigned cbyte = colok ? (unsigned)col * 4u : kOOB;
    float s = 0.f, q = 0.f;
    float bsc = 0.f, bsh = 0.f;          // BNR: this lane's column (read before the first store)
    if constexpr (BNR) {
        if (colok) { bsc = p.scale[col]; bsh = p.shift[col]; }
    }
    if constexpr (!BNS) {
    #pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int row0 = (e & 3) + 8 * (e >> 2);
            const unsigned ob0 = __builtin_amdgcn_readlane(obase, row0), ob1 = __builtin_amdgcn_readlane(obase, row0 + 4);
            const int of0 = __builtin_amdgcn_readlane(oflags, row0), of1 = __builtin_amdgcn_readlane(oflags, row0 + 4);
            const unsigned ob = kh ? ob1 : ob0;
            const int of = kh ? of1 : of0;
            float mm[16];
    #pragma unroll
            for (int xi = 0; xi < 16; ++xi) mm[xi] = acc[xi][e];
            // rows of A^T M: a0 = m0 + m1 + m2, a1 = m1 - m2 - m3 (over the first index), then the same over the second
            float a0[4], a1[4];
    #pragma unroll
            for (int j = 0; j < 4; ++j) {
                a0[j] = mm[j] + mm[4 + j] + mm[8 + j];
                a1[j] = mm[4 + j] - mm[8 + j] - mm[12 + j];
            }
            const float y[4] = {a0[0] + a0[1] + a0[2], a0[1] - a0[2] - a0[3], a1[0] + a1[1] + a1[2], a1[1] - a1[2] - a1[3]};
            // branch-free stores: a pixel outside the image or a column past Cout gets an out-of-range offset, which the
            // buffer store drops
            const bool live = ob != kOOB && colok;
            const bool ok[4] = {live, live && (of & 1), live && (of & 2), live && (of & 3) == 3};
            const unsigned off[4] = {ob, ob + right, ob + below, ob + below + right};
    #pragma unroll
            for (int k = 0; k < 4; ++k) {
                if constexpr (BNR) {
                    const float yy = fmaxf(fmaf(y[k], bsc, bsh), 0.f);
                    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, yy), srd_z, ok[k] ? off[k] + cbyte : kOOB, 0, 2 /* nt */);
                    continue;
                }
                if (!(p.flags & 1024))
                    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, y[k]), srd_z, ok[k] ? off[k] + cbyte : kOOB, 0, 2 /* nt */);
                const float u = ok[k] ? y[k] - pv : 0.f;
                s += u;
                q += u * u;
            }
        }

    } else {
        constexpr bool bns = true;
        const __amdgpu_buffer_rsrc_t srd_y = make_srd(bns ? p.y : p.z, p.z_bytes);
        // DS_EPI_BNSUMS (this launch is a dgrad whose result dy feeds a BatchNorm + ReLU backward): per column, the sums
        // of g = dy (y > 0) and g * y.  y sits at the offsets of the stores; (out-of-range
        // offsets read zeros: y = 0 drops the element from both sums).
        float yall[16][4];         // all sixty-four requested BEFORE the first store (a load behind a store waits for it)
        auto offsets_of = [&](int e, unsigned *off, bool *ok) {
            const int row0 = (e & 3) + 8 * (e >> 2);
            const unsigned ob0 = __builtin_amdgcn_readlane(obase, row0), ob1 = __builtin_amdgcn_readlane(obase, row0 + 4);
            const int of0 = __builtin_amdgcn_readlane(oflags, row0), of1 = __builtin_amdgcn_readlane(oflags, row0 + 4);
            const unsigned ob = kh ? ob1 : ob0;
            const int of = kh ? of1 : of0;
            // branch-free stores: a pixel outside the image or a column past Cout gets an out-of-range offset, which the
            // buffer store drops
            const bool live = ob != kOOB && colok;
            ok[0] = live; ok[1] = live && (of & 1); ok[2] = live && (of & 2); ok[3] = live && (of & 3) == 3;
            off[0] = ob; off[1] = ob + right; off[2] = ob + below; off[3] = ob + below + right;
        };
    #pragma unroll
        for (int e = 0; e < 16; ++e) {
            unsigned off[4];
            bool ok[4];
            offsets_of(e, off, ok);
    #pragma unroll
            for (int k = 0; k < 4; ++k)
                yall[e][k] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(srd_y, ok[k] ? off[k] + cbyte : kOOB, 0, 0));
        }
    #pragma unroll
        for (int e = 0; e < 16; ++e) {
            unsigned off[4];
            bool ok[4];
            offsets_of(e, off, ok);
            const float *ycur = yall[e];
            float mm[16];
    #pragma unroll
            for (int xi = 0; xi < 16; ++xi) mm[xi] = acc[xi][e];
            // rows of A^T M: a0 = m0 + m1 + m2, a1 = m1 - m2 - m3 (over the first index), then the same over the second
            float a0[4], a1[4];
    #pragma unroll
            for (int j = 0; j < 4; ++j) {
                a0[j] = mm[j] + mm[4 + j] + mm[8 + j];
                a1[j] = mm[4 + j] - mm[8 + j] - mm[12 + j];
            }
            const float y[4] = {a0[0] + a0[1] + a0[2], a0[1] - a0[2] - a0[3], a1[0] + a1[1] + a1[2], a1[1] - a1[2] - a1[3]};
    #pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (!(p.flags & 1024))
                    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, y[k]), srd_z, ok[k] ? off[k] + cbyte : kOOB, 0, 2 /* nt */);
                if (bns) {
                    const float u = (ok[k] && ycur[k] > 0.f) ? y[k] : 0.f;
                    s += u;
                    q += u * ycur[k];
                } else {
                    const float u = ok[k] ? y[k] - pv : 0.f;
                    s += u;
                    q += u * u;
                }
            }
        }

    }
    if (!BNR && (BNS || (p.flags & DS_EPI_STATS))) {
        float *red = smem;        // [4 waves][32][2]; every wave passed the last K-loop barrier, no DMA in flight
        s += __shfl_xor(s, 32);
        q += __shfl_xor(q, 32);
        if (kh == 0) {
            red[(wave * 32 + li) * 2 + 0] = s;
            red[(wave * 32 + li) * 2 + 1] = q;
        }
        __syncthreads();
        if (tid < 32 && co0 + tid < p.Cout) {
            float ss = 0.f, qq = 0.f;
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                ss += red[(w * 32 + tid) * 2 + 0];
                qq += red[(w * 32 + tid) * 2 + 1];
            }
            if (group < p.groups) {
                p.stats[(int64_t)(co0 + tid) * p.groups + group] = ss;
                p.stats[((int64_t)p.Cout + co0 + tid) * p.groups + group] = qq;
            }
        }
    }
}

// U = G g G^T for every (ci, co) pair.  w is the TF HWIO filter [3][3][Cin][Cout].
//   dgrad == 0: U[xi][co][ci] from g = w[:, :, ci, co]                       (forward)
//   dgrad == 1: U[xi][ci][co] from g = w[2 - kh, 2 - kw, ci, co]             (Conv2DBackpropInput: flipped taps,
//               output channel = ci, reduction channel = co)
__global__ __launch_bounds__(256) void wino_weights_kernel(const float *w, float *u, int Cin, int Cout, int dgrad) {
    const int64_t total = (int64_t)Cin * Cout;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int ci = (int)(i / Cout), co = (int)(i - (int64_t)ci * Cout);
        float g[3][3];
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b = 0; b < 3; ++b)
                g[a][b] = w[((int64_t)((dgrad ? 2 - a : a) * 3 + (dgrad ? 2 - b : b)) * Cin + ci) * Cout + co];
        float t[4][3];          // G g
#pragma unroll
        for (int b = 0; b < 3; ++b) {
            t[0][b] = g[0][b];
            t[1][b] = 0.5f * (g[0][b] + g[1][b] + g[2][b]);
            t[2][b] = 0.5f * (g[0][b] - g[1][b] + g[2][b]);
            t[3][b] = g[2][b];
        }
        const int64_t plane = total;
        const int64_t o = dgrad ? (int64_t)ci * Cout + co : (int64_t)co * Cin + ci;
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            u[(a * 4 + 0) * plane + o] = t[a][0];
            u[(a * 4 + 1) * plane + o] = 0.5f * (t[a][0] + t[a][1] + t[a][2]);
            u[(a * 4 + 2) * plane + o] = 0.5f * (t[a][0] - t[a][1] + t[a][2]);
            u[(a * 4 + 3) * plane + o] = t[a][2];
        }
    }
}

}  // namespace

extern "C" int ds_wino_transform_weights(const float *w, float *u, int32_t Cin, int32_t Cout, int32_t dgrad, void *stream) {
    DS_REQUIRE(w && u && Cin > 0 && Cout > 0, "ds_wino_transform_weights: bad argument");
    hipLaunchKernelGGL(wino_weights_kernel, dim3(ds::stream_grid((int64_t)Cin * Cout, 256)), dim3(256), 0,
                       (hipStream_t)stream, w, u, Cin, Cout, dgrad);
    return ds::check_launch("ds_wino_transform_weights");
}

namespace { int g_allow_ablation = 0; }

// Debug aid (process-global, never called by the product path): let ds_conv_wino accept its ablation flag bits.
#ifdef DS_TUNING
extern "C" int ds_debug_conv_wino_allow_ablation(int on) {
    g_allow_ablation = on ? 1 : 0;
    return DS_OK;
}
#endif

extern "C" int ds_conv_wino_partials(int32_t N, int32_t H, int32_t W) {
    const int64_t mt = (int64_t)N * ((H + 1) / 2) * ((W + 1) / 2);
    return (int)((mt + 127) / 128);
}

namespace {
int wino_launch(const float *x, const float *u, float *z, float *stats, const float *pivot, const float *ymask, const float *scale,
                const float *shift, int32_t N, int32_t H, int32_t W, int32_t Cin, int32_t ldx, int32_t Cout, int32_t ldz,
                int32_t flags, void *stream);
}

extern "C" int ds_conv_wino(const float *x, const float *u, float *z, float *stats, const float *pivot, const float *ymask,
                            int32_t N, int32_t H, int32_t W, int32_t Cin, int32_t ldx, int32_t Cout, int32_t ldz,
                            int32_t flags, void *stream) {
    DS_REQUIRE(!(flags & DS_EPI_BN_RELU), "ds_conv_wino: DS_EPI_BN_RELU takes its scale / shift through ds_conv_run (ds_conv_io)");
    return wino_launch(x, u, z, stats, pivot, ymask, nullptr, nullptr, N, H, W, Cin, ldx, Cout, ldz, flags, stream);
}

// ds_conv_run's entry for DS_EPI_BN_RELU plans of this family
namespace ds {
int conv_wino_bn_relu(const float *x, const float *u, float *z, const float *scale, const float *shift, int32_t N, int32_t H,
                      int32_t W, int32_t Cin, int32_t ldx, int32_t Cout, int32_t ldz, void *stream) {
    DS_REQUIRE(scale && shift, "ds_conv_run: DS_EPI_BN_RELU without scale / shift");
    return wino_launch(x, u, z, nullptr, nullptr, nullptr, scale, shift, N, H, W, Cin, ldx, Cout, ldz, DS_EPI_BN_RELU, stream);
}
}  // namespace ds

namespace {
int wino_launch(const float *x, const float *u, float *z, float *stats, const float *pivot, const float *ymask, const float *scale,
                const float *shift, int32_t N, int32_t H, int32_t W, int32_t Cin, int32_t ldx, int32_t Cout, int32_t ldz,
                int32_t flags, void *stream) {
    DS_REQUIRE(x && u && z && N > 0 && H > 0 && W > 0, "ds_conv_wino: bad argument");
    const bool bnr = (flags & DS_EPI_BN_RELU) != 0;
    DS_REQUIRE(!bnr || (flags == DS_EPI_BN_RELU && scale && shift), "ds_conv_wino: DS_EPI_BN_RELU excludes every other flag and needs scale / shift");
    if (bnr) flags = 0;          // (the checks below and the kernel's flag word know the training epilogues only)
    DS_REQUIRE(Cin > 0 && Cin % 8 == 0 && ldx % 4 == 0 && ldx >= Cin && Cout > 0 && ldz >= Cout &&
                   ((((uintptr_t)x | (uintptr_t)u) & 15) == 0),
               "ds_conv_wino: needs Cin %% 8 == 0, ldx %% 4 == 0 and 16-byte aligned operands");
    // bits 256 / 512 / 1024 / 2048 are ablation switches of the kernel (skip the pixel loads / the weight DMAs / the output
    // stores ...: the results are garbage); they are refused unless ds_debug_conv_wino_allow_ablation(1) was called, so a
    // stray bit in `flags` fails here instead of "succeeding" with an unwritten z (ds_conv_wino4 refuses them always)
    const int32_t ablation = g_allow_ablation ? (256 | 512 | 1024 | 2048) : 0;
    DS_REQUIRE((flags & ~(DS_EPI_STATS | DS_EPI_BNSUMS | ablation)) == 0 && (!(flags & (DS_EPI_STATS | DS_EPI_BNSUMS)) || stats),
               "ds_conv_wino: only DS_EPI_STATS / DS_EPI_BNSUMS are supported (with a partials buffer)");
    DS_REQUIRE(!(flags & DS_EPI_BNSUMS) || (ymask && !(flags & DS_EPI_STATS)),
               "ds_conv_wino: DS_EPI_BNSUMS needs y (pixel stride ldz) and excludes DS_EPI_STATS");
    WinoParams p;
    p.x = x; p.u = u; p.z = z; p.stats = stats; p.pivot = (flags & DS_EPI_STATS) ? pivot : nullptr;
    p.y = (flags & DS_EPI_BNSUMS) ? ymask : nullptr;
    p.scale = scale; p.shift = shift;
    p.N = N; p.H = H; p.W = W; p.Cin = Cin; p.ldx = ldx; p.Cout = Cout; p.ldz = ldz;
    p.TH = (H + 1) / 2; p.TW = (W + 1) / 2;
    const int64_t mt = (int64_t)N * p.TH * p.TW;
    const int64_t xb = ((int64_t)N * H * W - 1) * ldx + Cin, ub = (int64_t)16 * Cin * Cout;
    DS_REQUIRE(mt < (1ll << 30) && xb * 4 < (1ll << 31) && ub * 4 < (1ll << 31), "ds_conv_wino: operand larger than 2 GiB");
    p.Mt = (int)mt;
    p.x_bytes = (unsigned)(xb * 4);
    p.u_bytes = (unsigned)(ub * 4);
    const int64_t zb = ((int64_t)N * H * W - 1) * ldz + Cout;
    DS_REQUIRE(zb * 4 < (1ll << 31), "ds_conv_wino: output larger than 2 GiB");
    p.z_bytes = (unsigned)(zb * 4);
    p.flags = flags;
    p.groups = (int)((mt + 127) / 128);
    p.ncol = (Cout + 31) / 32;
    const dim3 grid((unsigned)(((int64_t)p.groups * p.ncol + 7) / 8 * 8));
    if (bnr) hipLaunchKernelGGL((conv_wino_kernel<false, true>), grid, dim3(256), 0, (hipStream_t)stream, p);
    else if (flags & DS_EPI_BNSUMS) hipLaunchKernelGGL(conv_wino_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, p);
    else hipLaunchKernelGGL(conv_wino_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, p);
    return ds::check_launch("ds_conv_wino");
}
}  // namespace
