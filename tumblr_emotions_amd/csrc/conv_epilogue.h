// What the convolution kernels share on their way out (internal): the buffer-descriptor helpers, and the two epilogues of the
// 32x32-MFMA kernels -- bias / accumulate / mask / relu, the store, BatchNorm column statistics.
//   * tile epilogue (a workgroup's waves stacked along M, plain pointer stores): tile_store + tile_stats_combine, called by
//     igemm_workgroup (conv_igemm_kernel, gemm_group_kernel) and conv_glds_kernel;
//   * wave-row epilogue (one wave per 32 rows x NB * 32 columns, descriptor addressing, reads before stores): wave_row_epilogue,
//     called by gemm_wide_kernel and conv_bf16d_kernel.
// A difference between callers is either a compile-time option or an argument; the comment at each says which.
// conv_bf16_kernel and conv_fp8d_kernel hold the same code in place: on the shared functions their schedule or
// occupancy moved (profiles/conv_epilogue_notes.md).  Of the callers, conv_igemm_kernel<1, 1, false, false, *> gained a wave per
// SIMD, so its persistent launches (more than 2048 row tiles) have a larger grid.
#pragma once
#include "ds_common.h"

namespace ds {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr unsigned kOOB = 0x80000000u;   // byte offset beyond any descriptor: a load returns 0, a store is dropped

__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_srd(const void *p, unsigned bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(p), 0, (int)bytes, 0x00020000);
}

// row of accumulator element r of a 32x32 MFMA tile, for the lanes of the lower half-wave (the upper half: + 4)
__device__ __forceinline__ constexpr int acc_row(int r) { return (r & 3) + 8 * (r >> 2); }

// ---- tile epilogue ---------------------------------------------------------------------------------------------------------
// Store phase of a lane's share of a tile: acc(a, b), a < MT, b < NT, are its 32x32 accumulators (MT stacked along M, NT column
// blocks), row0 its first row of acc(0, .) (tile origin + wave origin + 4 * (lane >> 5)), col0 its column of block 0, zout the
// output or a split-K launch's slab.  bias and pivot are read once per column; the columns' sums about the pivot are added to
// csum / csq.  The column loop is in here, and M, the descriptor and the pointers are arguments read at the call in the epilogue:
// with one call per column block (or the fields copied in front of the K loop) the compiler hoists a tile's sixteen 64-bit row
// offsets out of the column loop and keeps them alive across it -- +40 registers, the 128 x 64 tile fell from five waves per
// SIMD to three.
// BNR (compile time: its own instantiations, so the training kernels' code is untouched): DS_EPI_BN_RELU, scale / shift once
// per column and y = max(fma(acc, scale, shift), 0) stored in place of z; nothing else, no sums.
template <int MT, int NT, bool BNR, class Acc>
__device__ __forceinline__ void tile_store(const ds_conv_desc &d, int M, float *zout, const float *bias, const float *mask,
                                           const float *pivot, const float *scale, const float *shift, Acc acc, int row0, int col0,
                                           float (&csum)[NT], float (&csq)[NT]) {
    const int flags = d.flags;
#pragma unroll
    for (int b = 0; b < NT; ++b) {
        const int col = col0 + b * 32;
        const bool colok = col < d.Cout;
        if constexpr (BNR) {
            const float sc = colok ? scale[col] : 0.f, sh = colok ? shift[col] : 0.f;
#pragma unroll
            for (int a = 0; a < MT; ++a) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = row0 + a * 32 + acc_row(r);
                    if (row < M && colok) zout[(int64_t)row * d.ldz + col] = fmaxf(fmaf(acc(a, b)[r], sc, sh), 0.f);
                }
            }
            continue;
        }
        const float bv = ((flags & DS_EPI_BIAS) && colok) ? bias[col] : 0.f;
        const float pv = (pivot && colok) ? pivot[col] : 0.f;      // statistics are taken about the pivot
        float s = 0.f, q = 0.f;
#pragma unroll
        for (int a = 0; a < MT; ++a) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = row0 + a * 32 + acc_row(r);
                if (row < M && colok) {
                    float v = acc(a, b)[r] + bv;
                    const int64_t off = (int64_t)row * d.ldz + col;
                    if (flags & DS_EPI_ACCUM) v += zout[off];
                    if (flags & DS_EPI_MASK) v = mask[(int64_t)row * d.ldmask + col] > 0.f ? v : 0.f;
                    if (flags & DS_EPI_RELU) v = fmaxf(v, 0.f);
                    zout[off] = v;
                    const float u = v - pv;
                    s += u;
                    q += u * u;
                }
            }
        }
        csum[b] += s;
        csq[b] += q;
    }
}

// Statistics combine of a workgroup of 4 waves stacked along M: rows of a column live in lanes l and l ^ 32 and in the four
// waves.  red: [4][NT * 32][2] floats of LDS that every wave is done with once it arrives here (the leading barrier).
// Partials are laid out [2][Cout][P] (P = workgroups per column tile) so that ds_bn_finalize reads them contiguously; this
// workgroup's is number `part`.  item (argument): the workgroup owned a tile at all.
template <int NT>
__device__ __forceinline__ void tile_stats_combine(float *red, const float (&csum)[NT], const float (&csq)[NT], int n0, int Cout,
                                                   bool item, float *stats, int P, int part) {
    constexpr int BN = NT * 32;
    const int tid = threadIdx.x, li = tid & 31, lk = (tid >> 5) & 1;
    const int wm = __builtin_amdgcn_readfirstlane(tid >> 6);
    __syncthreads();
#pragma unroll
    for (int b = 0; b < NT; ++b) {
        const float s = csum[b] + __shfl_xor(csum[b], 32);
        const float q = csq[b] + __shfl_xor(csq[b], 32);
        if (lk == 0) {
            const int c = b * 32 + li;
            red[(wm * BN + c) * 2 + 0] = s;
            red[(wm * BN + c) * 2 + 1] = q;
        }
    }
    __syncthreads();
    if (tid < BN && n0 + tid < Cout && item) {
        float s = 0.f, q = 0.f;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            s += red[(w * BN + tid) * 2 + 0];
            q += red[(w * BN + tid) * 2 + 1];
        }
        stats[(int64_t)(n0 + tid) * P + part] = s;
        stats[((int64_t)Cout + n0 + tid) * P + part] = q;
    }
}

// ---- wave-row epilogue -----------------------------------------------------------------------------------------------------
// Compile-time options: what a kernel's epilogue HAS.  What a launch asks for -- the flags, 16-bit storage, mask_rstd -- stays
// a wave-uniform runtime branch, so the instantiation count is the kernels' own.
struct WaveRowOpt {        // a kernel's options type derives from this and redefines what it has
    static constexpr bool bnr = false;         // DS_EPI_BN_RELU: scale / shift read in phase 1, relu(fma) at the store, nothing else (wide)
    static constexpr bool half = false;        // 16-bit storage exists: d.mask_dtype / d.z_dtype are honoured (bf16d)
    static constexpr bool mask_rstd = false;   // d.mask_rstd / mask_shift are honoured (wide, bf16d)
};

// Arguments that differ between callers:
//   mrow0, Mrow   the wave's first row and the row bound: rows >= Mrow do not exist.  wide: Mw, under POOL the wave's last real
//                 row + 1; bf16d: M.  The z and activation descriptors end with row Mrow - 1;
//   any_row       false: the wave has no row at all and its descriptors are empty (wide under POOL; the others pass true);
//   trow, P       the workgroup's row tile and the partial count: stats[2][Cout][P];
//   red           [4][32][2] floats of LDS nothing else uses any more;
//   wave, li, kh  the kernel's own: wave of the workgroup (uniform), lane & 31, lane >> 5;
//   scale, shift  bnr.
// Two phases.  (1) per column block: the accumulate / activation reads -- the sixteen of a block requested together -- the
// sums, the LDS combine (two barriers, with statistics only); results stay in the accumulator registers.  (2) all stores,
// then the partials.  With the stores of block b in front of the reads of block b + 1 every block cost a memory round trip
// (a load behind a store waits for it: one in-order counter).
// z (and the reads at the same rows and columns) through buffer descriptors: ONE 32-bit lane offset per column block plus the
// row's wave-uniform byte offset, added into the VECTOR offset (the scalar offset of a buffer instruction is not
// range-checked); rows past Mrow and columns past Cout (offset kOOB = 2^31, which the row offsets cannot wrap) fall out of
// the descriptor's range: loads return 0, stores are dropped.  (Outputs of 2 GiB and more stay on the LDS-tile kernels.)
template <int NB, class O>
__device__ __forceinline__ void wave_row_epilogue(f32x16 (&acc)[NB], const ds_conv_desc &d, float *z, const float *mask, float *stats,
                                                  const float *pivot, bool item, int n0, int mrow0, int Mrow, bool any_row, int trow,
                                                  int P, float *red, int wave, int li, int kh, const float *scale,
                                                  const float *shift) {
    const int tid = threadIdx.x;
    const int flags = d.flags;
    const bool m16 = O::half && d.mask_dtype == DS_DTYPE_BF16;      // (uniform) BatchNorm-sums activation in bf16 storage
    const bool z16 = O::half && d.z_dtype == DS_DTYPE_BF16;         // (uniform) z stored as bf16(z - pivot) (forward, no accumulate)
    const unsigned zeb = z16 ? 2u : 4u, meb = m16 ? 2u : 4u;
    const __amdgpu_buffer_rsrc_t srd_z = make_srd(z, any_row ? (unsigned)(((int64_t)(Mrow - 1) * d.ldz + d.Cout) * zeb) : 0u);
    const __amdgpu_buffer_rsrc_t srd_m = make_srd((flags & DS_EPI_BNSUMS) ? (const void *)mask : (const void *)z,
                                                  ((flags & DS_EPI_BNSUMS) && any_row) ? (unsigned)(((int64_t)(Mrow - 1) * d.ldmask + d.Cout) * meb) : 0u);
    const int rz = d.ldz * (int)zeb, rm = d.ldmask * (int)meb;      // bytes per row
    const int rbase = mrow0 + 4 * kh;                               // this lane's first row; accumulator element r: + acc_row(r)
    float pss[NB], pqq[NB];                              // (threads 0..31) this workgroup's partials of column block b
    float bsc[O::bnr ? NB : 1], bsh[O::bnr ? NB : 1];      // bnr: scale / shift of this lane's column of block b
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        const int col = n0 + 32 * b + li;
        const bool colok = item && col < d.Cout;
        if constexpr (O::bnr) {
            bsc[b] = colok ? scale[col] : 0.f;
            bsh[b] = colok ? shift[col] : 0.f;
            pss[b] = pqq[b] = 0.f;
            continue;
        }
        const float pv = (pivot && colok) ? pivot[col] : 0.f;
        const unsigned vz = colok ? (unsigned)(rbase * d.ldz + col) * zeb : kOOB;
        const unsigned vm = colok ? (unsigned)(rbase * d.ldmask + col) * meb : kOOB;
        float s = 0.f, q = 0.f;
        if (flags & DS_EPI_ACCUM) {               // the sixteen previous values, requested together
            float zv[16];
#pragma unroll
            for (int r = 0; r < 16; ++r)
                zv[r] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(srd_z, vz + (unsigned)(acc_row(r) * rz), 0, 0));
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[b][r] += zv[r];
        }
        if (flags & DS_EPI_BNSUMS) {
            // dgrad whose result dy feeds a BatchNorm + ReLU backward: column sums of g = dy (y > 0) and g * y, y = the
            // consumer layer's forward activation (same rows / columns as dy; fp32, or bf16 under 16-bit activation storage)
            float yv[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const unsigned v = vm + (unsigned)(acc_row(r) * rm);
                if (m16) yv[r] = __builtin_bit_cast(float, (unsigned)__builtin_amdgcn_raw_buffer_load_b16(srd_m, v, 0, 0) << 16);
                else yv[r] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(srd_m, v, 0, 0));
            }
            if constexpr (O::mask_rstd) {
                if (d.mask_rstd && colok) {      // `mask` holds z of the consumer layers: y = relu(z * rstd + shift) per column
                    const float mr = d.mask_rstd[col], ms = d.mask_shift[col];
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int row = rbase + acc_row(r);
                        yv[r] = row < Mrow ? fmaxf(fmaf(yv[r], mr, ms), 0.f) : 0.f;      // (rows past M read 0, which a shift > 0 would turn on)
                    }
                }
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float u = yv[r] > 0.f ? acc[b][r] : 0.f;          // (out of range: y = 0)
                s += u;
                q += u * yv[r];
            }
        } else if (flags & DS_EPI_STATS) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = rbase + acc_row(r);
                if (row < Mrow && colok) {
                    const float u = acc[b][r] - pv;
                    s += u;
                    q += u * u;
                }
            }
        }
        pss[b] = pqq[b] = 0.f;
        if (flags & (DS_EPI_STATS | DS_EPI_BNSUMS)) {
            s += __shfl_xor(s, 32);
            q += __shfl_xor(q, 32);
            __syncthreads();
            if (kh == 0) {
                red[(wave * 32 + li) * 2 + 0] = s;
                red[(wave * 32 + li) * 2 + 1] = q;
            }
            __syncthreads();
            if (tid < 32) {
#pragma unroll
                for (int w = 0; w < 4; ++w) {
                    pss[b] += red[(w * 32 + tid) * 2 + 0];
                    pqq[b] += red[(w * 32 + tid) * 2 + 1];
                }
            }
        }
    }
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        const int col = n0 + 32 * b + li;
        const bool colok = item && col < d.Cout;
        const unsigned vz = colok ? (unsigned)(rbase * d.ldz + col) * zeb : kOOB;
        if (z16) {
            // z CENTRED about the pivot before it is rounded: the BatchNorm passes use z - mean, and for a channel with
            // |mean| >> sigma a bf16 z would carry (|mean| / sigma) 2^-9 of error into xhat; z - pivot (pivot = the previous
            // step's mean) is of the size of sigma, its rounding error 2^-9 of xhat itself.  The consumers get mean - pivot and
            // beta - (mean - pivot) rstd (ds_bn_finalize_centered)
            const float pvz = (pivot && colok) ? pivot[col] : 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const __bf16 hv = (__bf16)(acc[b][r] - pvz);          // round to nearest even
                __builtin_amdgcn_raw_buffer_store_b16(__builtin_bit_cast(unsigned short, hv), srd_z, vz + (unsigned)(acc_row(r) * rz), 0, 2 /* nt */);
            }
        } else {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                // (bit_cast of a vector-element lvalue reads element 0: copy first)
                const float val = O::bnr ? fmaxf(fmaf(acc[b][r], bsc[b], bsh[b]), 0.f) : acc[b][r];
                __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, val), srd_z, vz + (unsigned)(acc_row(r) * rz), 0, 2 /* nt */);
            }
        }
        if ((flags & (DS_EPI_STATS | DS_EPI_BNSUMS)) && tid < 32 && item && n0 + 32 * b + tid < d.Cout) {
            float *const sp = stats + (int64_t)(n0 + 32 * b + tid) * P + trow;
            float *const qp = stats + ((int64_t)d.Cout + n0 + 32 * b + tid) * P + trow;
            *sp = pss[b];
            *qp = pqq[b];
        }
    }
}

}  // namespace ds
