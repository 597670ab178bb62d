// Shared helpers for the gfx950 kernel library (internal; the public ABI is include/ds_kernels.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include "ds_kernels.h"

namespace ds {

void set_error(const char *fmt, ...);

// Tuning knobs (DS_* environment variables read by the selection rules: tile pins, cost-model coefficients, A/B switches)
// exist in the -DDS_TUNING build only (libds_kernels_tuning.so, what scripts/ and the kernel tests load); the shipped
// library reads no environment variable and every knob has its default.
#ifdef DS_TUNING
inline const char *tune_env(const char *name) { return getenv(name); }
#else
inline const char *tune_env(const char *) { return nullptr; }
#endif

inline int check_launch(const char *what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_error("%s: %s", what, hipGetErrorString(e));
        return DS_ERR_LAUNCH;
    }
    return DS_OK;
}

// MI355X: 256 CUs in 8 XCDs.  Memory-bound kernels cap their grid at 8 blocks per CU and
// grid-stride the rest (cdna_hip_programming.md Guideline 11).
constexpr int kCUs = 256;
constexpr int kMaxStreamBlocks = kCUs * 8;

// grid of the grid-stride streaming kernels (pools, copies, reductions): at most kMaxStreamBlocks workgroups
// (DS_STREAM_MAX = workgroups per CU, tuning library only)
inline int stream_grid(int64_t work_items, int per_block) {
    static int cap = 0;
    if (!cap) {
        const char *e = tune_env("DS_STREAM_MAX");
        cap = e && atoi(e) > 0 ? kCUs * atoi(e) : kMaxStreamBlocks;
    }
    int64_t b = (work_items + per_block - 1) / per_block;
    if (b < 1) b = 1;
    if (b > cap) b = cap;
    return (int)b;
}

// 16-byte load of data that is read once (streaming): non-temporal hint, so the lines do not displace what the
// neighbouring kernels keep in L2 / the Infinity Cache (scripts/microbench/stream_bw.hip)
typedef float f32x4_nt __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float4 ld_stream4(const float *p) {
    const f32x4_nt v = __builtin_nontemporal_load(reinterpret_cast<const f32x4_nt *>(p));
    return make_float4(v.x, v.y, v.z, v.w);
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// *word = max(*word, v) for non-negative floats (they order like unsigned integers, so the result is exact and
// independent of the order).  Thousands of waves aim at one word: each first LOOKS at it (an agent-scope load, served by
// L2) and only the few whose value still exceeds it pay for the atomic -- with the plain atomic per wave the BatchNorm
// apply kernels ran 3-6x longer.
// A max|.| RECORD is DS_AMAX_FLOATS floats: 16 slots, one per 128-byte line, so that the waves of a launch spread over
// 16 L2 lines instead of queueing on one word; the reader takes the maximum of the 16 slots (amax_read).
__device__ __forceinline__ void atomic_max_nonneg(float *record, float v) {
    if (!(v > 0.f)) return;
    const unsigned bits = __float_as_uint(v);
    const unsigned slot = (blockIdx.x + (threadIdx.x >> 6)) & 15u;
    unsigned *w = reinterpret_cast<unsigned *>(record) + 32u * slot;
    if (__hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= bits) return;
    atomicMax(w, bits);
}

// max over the 16 slots of a record (every lane gets it); a finished producer launch is assumed (stream order)
__device__ __forceinline__ float amax_read(const float *record) {
    float m = record[32 * (threadIdx.x & 15)];
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    return m;
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// slim.batch_norm (scale = False) + ReLU backward for one element: dz from the layer's pre-BatchNorm z, the gradient dy of
// its activation and the per-channel rstd r, shift s, mean mu, column means a1 = mean(g), a2 = mean(g xhat).  ONE
// definition, explicit fused multiply-adds: ds_bn_bwd_apply and the wide dgrad's on-load form give the same bits.
__device__ __forceinline__ float bn_bwd_dz(float z, float dy, float r, float s, float mu, float a1, float a2) {
    const float g = __builtin_fmaf(z, r, s) > 0.f ? dy : 0.f;
    const float xh = (z - mu) * r;
    return r * __builtin_fmaf(-xh, a2, g - a1);
}

__device__ __forceinline__ void ld_vec4(float (&v)[4], const float *p) {
    const float4 t = *reinterpret_cast<const float4 *>(p);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
}

// Per-element functor of the BatchNorm-backward walks (bn.hip: bn_row_walk over dense rows, pool.hip: pool_patch_walk over
// the 2x2 patches of a stride-2 pool) for the moving-statistics backward: dz = rstd * g * [z*rstd + shift > 0], stored
// non-temporally where z has the element (dz has z's layout; it may be z).  The predicate is the fused multiply-add
// bn_apply_relu_kernel evaluates, so the mask has the decision bits of the activation the forward pass wrote.
// SUMS: also the thread's column sums of g * [..] in walk order (frozen-BatchNorm training: dbeta), for
// combine_column_groups.  WRITE = false: only the sums are wanted.
// A walk calls channel(c) for the thread's float4 column group and element(z[4], g[4], c, row / pixel index, offset of the z
// element) once per row / pixel.
template <bool WRITE, bool SUMS>
struct InferBwd {
    static constexpr bool kStreamZ = true, kHoist = SUMS;      // (pool_patch_walk)
    const float *rstd, *shift;
    float *dz;
    float rr[4], ss[4], sum[4];
    __device__ __forceinline__ void channel(int c) {
        ld_vec4(rr, rstd + c);
        ld_vec4(ss, shift + c);
#pragma unroll
        for (int j = 0; j < 4; ++j) sum[j] = 0.f;
    }
    __device__ __forceinline__ void element(const float (&z)[4], const float (&g)[4], int, int64_t, int64_t zoff) {
        f32x4_nt o;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool on = __builtin_fmaf(z[j], rr[j], ss[j]) > 0.f;
            if (SUMS) sum[j] += on ? g[j] : 0.f;
            o[j] = on ? rr[j] * g[j] : 0.f;
        }
        if (WRITE) __builtin_nontemporal_store(o, reinterpret_cast<f32x4_nt *>(dz + zoff));
    }
};

// The workgroup's column sums of a walk in which thread t of workgroup b keeps column group (256 b + t) mod C4: `mine` holds
// the thread's PLANES x 4 sums (plane k in [4k, 4k + 4)).  The owner of a column group -- thread cg, cg + 256, ... -- adds the
// group's threads in thread order and stores partials[k][4 cg + j][b]: float[PLANES][C][P], P = gridDim.x.  A column group the
// workgroup does not meet (C4 > 256) gets an exact 0, so every slot is written by every launch.  No atomics.
template <int PLANES>
__device__ __forceinline__ void combine_column_groups(float (*sh)[4 * PLANES], const float (&mine)[4 * PLANES], int C4, int C,
                                                      float *partials) {
#pragma unroll
    for (int j = 0; j < 4 * PLANES; ++j) sh[threadIdx.x][j] = mine[j];
    __syncthreads();
    const int P = gridDim.x;
    const int head = (int)(((int64_t)blockIdx.x * 256) % C4);      // column group of this workgroup's thread 0
    for (int cg = threadIdx.x; cg < C4; cg += 256) {
        int t0 = cg - head;
        if (t0 < 0) t0 += C4;
        float a[4 * PLANES];
#pragma unroll
        for (int j = 0; j < 4 * PLANES; ++j) a[j] = 0.f;
        for (int t = t0; t < 256; t += C4)
#pragma unroll
            for (int j = 0; j < 4 * PLANES; ++j) a[j] += sh[t][j];
#pragma unroll
        for (int k = 0; k < PLANES; ++k)
#pragma unroll
            for (int j = 0; j < 4; ++j) partials[((int64_t)k * C + cg * 4 + j) * P + blockIdx.x] = a[4 * k + j];
    }
}

}  // namespace ds

#define DS_REQUIRE(cond, ...)                 \
    do {                                      \
        if (!(cond)) {                        \
            ds::set_error(__VA_ARGS__);       \
            return DS_ERR_ARG;                \
        }                                     \
    } while (0)
