// Conv2DBackpropInput of Conv2d_1a_7x7 (image_model/inception_v1.py:63: 7x7, stride 2, SAME, 3 -> 64 channels): the
// gradient of the packed RGB images, what gradient ascent on the input (class_visualisation) and saliency maps need.
//
//   dx[n, ih, iw, c] = sum_{kh, kw, co} dz[n, oh, ow, co] w[kh][kw][c][co],   ih = 2 oh - pad_t + kh,  iw = 2 ow - pad_l + kw
//
// Only 3 output channels exist, so a matrix-core tile with N = 3 would idle 81-90 % of its columns; on gfx950 the fp32 VALU
// (v_pk_fma_f32) peaks at the same 64 FLOP/clk/SIMD as the fp32 MFMA, so this is a VALU gather kernel:
//   * for an input pixel only the taps with kh = (ih + pad_t) mod 2 (mod 2) and likewise kw meet a whole output pixel: 4 x 4,
//     4 x 3, 3 x 4 or 3 x 3 taps by the pixel's PARITY CLASS.  A 256-thread workgroup owns a 32 x 32 input tile; wave w owns
//     parity class (w >> 1, w & 1) -- the taps are wave-uniform, so the filter is read with broadcast LDS reads -- and a lane
//     owns a 2 x 2 block of that class (pixels two rows / columns apart), whose 4 (x 4) taps fall on a 5 x 5 window of dz;
//   * dz of the tile (20 x 20 output pixels) is staged in LDS 16 channels at a time (the next slice is fetched into registers
//     while the current one is used); the whole filter sits in LDS in pair order (below), loaded once per persistent
//     workgroup from the HWIO store (the 4th input channel of a zero-padded store is never read);
//   * per 4 channels and lane: 25 ds_read_b128 of dz, 3 broadcast ds_read_b128 of the filter per tap, 6 v_pk_fma_f32 per tap
//     and pixel -- channels 0 / 1 of one dz value in one packed FMA, channel 2 of two dz values in another;
//   * one lane writes each dx element, no atomics: the result does not depend on the launch shape.
// Measured alternative, not kept: the filter through scalar loads straight from the HWIO store (SGPR operands of the packed
// FMAs, no filter in LDS, 32 KB of LDS) ran 1041 us at B = 256 against 928-935 us for this form.
#include "ds_common.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

namespace {

constexpr int CO = 64;
constexpr int TI = 32;            // input tile (rows and columns) of a workgroup
constexpr int TR = 20;            // output rows / columns of dz a tile reads (TI / 2 + 3, + 1 for pad_t = 3)
constexpr int CK = 16;            // channels of dz per LDS slice
constexpr int PS = CK + 4;        // floats per staged dz pixel (padded: lanes two pixels apart use other banks)
constexpr int NSLICE = CO / CK;
constexpr int FETCH = (TR * TR * (CK / 4) + 255) / 256;      // 16-byte loads per thread and slice
constexpr int WFLOATS = 49 * CO * 3;                          // the filter, 7 x 7 taps x 64 x 3

struct DgradParams {
    const float *dz;     // [N, OH, OW, ldx]
    const float *w;      // HWIO [7][7][cin_store][64]
    float *dx;           // [N, H, W, 3]
    int N, H, W, OH, OW, pad_t, pad_l, cin_store, ldx;
    int tiles_h, tiles_w, tiles;
};

__device__ __forceinline__ int floor_half(int v) { return v >= 0 ? v / 2 : -((1 - v) / 2); }

__device__ __forceinline__ f32x2 pk_fma(f32x2 a, f32x2 b, f32x2 c) { return __builtin_elementwise_fma(a, b, c); }

// acc[i][j] (pixel rows i, columns j of the lane's 2 x 2 block): {c0, c1} in a / b (two chains), {c2 of even, odd channel} in e
struct Acc { f32x2 a[2][2], b[2][2], e[2][2]; };

// the taps of one parity class (NT x NS of them) over a staged slice: d = the lane's 5 x 5 window, wt = filter of the tap
// (kh0 + 2 t, kw0 + 2 s)
template <int NT, int NS>
__device__ __forceinline__ void class_slice(const float *__restrict__ dzl, const float *__restrict__ wl, int lane_off, int kh0,
                                            int kw0, int co0, Acc &acc) {
#pragma unroll 1
    for (int g = 0; g < CK / 4; ++g) {
        // (the window is read in the order the taps use it -- rows and columns from the far end -- and the filter of tap
        // k + 1 is requested before the FMAs of tap k: the LDS latency passes under arithmetic instead of in front of it)
        f32x4 d[5][5];
#pragma unroll
        for (int r = 4; r >= 4 - NT; --r)
#pragma unroll
            for (int c = 4; c >= 4 - NS; --c)
                d[r][c] = *reinterpret_cast<const f32x4 *>(dzl + lane_off + (r * TR + c) * PS + 4 * g);
        const float *wg = wl + (co0 + 4 * g) * 3;
        f32x4 W[2][3];
        auto wload = [&](int k, f32x4 (&dst)[3]) {
            const float *wt = wg + ((kh0 + 2 * (k / NS)) * 7 + kw0 + 2 * (k % NS)) * (CO * 3);
            dst[0] = *reinterpret_cast<const f32x4 *>(wt);
            dst[1] = *reinterpret_cast<const f32x4 *>(wt + 4);
            dst[2] = *reinterpret_cast<const f32x4 *>(wt + 8);
        };
        wload(0, W[0]);
#pragma unroll
        for (int k = 0; k < NT * NS; ++k) {
            const int t = k / NS, s = k % NS;
            if (k + 1 < NT * NS) wload(k + 1, W[(k + 1) & 1]);
            const f32x4 W0 = W[k & 1][0], W1 = W[k & 1][1], W2 = W[k & 1][2];
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const f32x4 v = d[3 + i - t][3 + j - s];
                    acc.a[i][j] = pk_fma(f32x2{v.x, v.x}, W0.xy, acc.a[i][j]);
                    acc.b[i][j] = pk_fma(f32x2{v.y, v.y}, W0.zw, acc.b[i][j]);
                    acc.e[i][j] = pk_fma(v.xy, W1.xy, acc.e[i][j]);
                    acc.a[i][j] = pk_fma(f32x2{v.z, v.z}, W1.zw, acc.a[i][j]);
                    acc.b[i][j] = pk_fma(f32x2{v.w, v.w}, W2.xy, acc.b[i][j]);
                    acc.e[i][j] = pk_fma(v.zw, W2.zw, acc.e[i][j]);
                }
        }
    }
}

__global__ __launch_bounds__(256, 2) void conv_stem_dgrad_kernel(const DgradParams p) {
    // filter in pair order: [kh][kw][co pair q][6] = w0[2q], w1[2q], w0[2q+1], w1[2q+1], w2[2q], w2[2q+1] -- four channels are
    // three aligned float4 of one tap (W0 = {w0, w1 of co}, {w0, w1 of co + 1}; W1 = {w2 of co, co + 1}, {w0, w1 of co + 2};
    // W2 = {w0, w1 of co + 3}, {w2 of co + 2, co + 3})
    __shared__ __attribute__((aligned(16))) float wl[WFLOATS];
    __shared__ __attribute__((aligned(16))) float dzl[TR * TR * PS];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    for (int i = tid; i < WFLOATS; i += 256) {
        const int tap = i / (CO * 3), r = i - tap * (CO * 3);
        const int quad = r / 12, k = r - quad * 12;
        // k -> (channel offset inside the quad, input channel)
        const int dco = (k < 4) ? (k >> 1) : (k < 6) ? (k - 4) : (k < 8) ? 2 : (k < 10) ? 3 : (k - 10 + 2);
        const int c = (k < 4) ? (k & 1) : (k < 6) ? 2 : (k < 10) ? (k & 1) : 2;
        wl[i] = p.w[(tap * p.cin_store + c) * CO + quad * 4 + dco];
    }
    const int pr = wave >> 1, pc = wave & 1;      // the wave's parity class inside the tile (tile origins are even)
    const int la = lane >> 3, lb = lane & 7;       // the lane's 2 x 2 block: pixels (pr + 4 la + 2 i, pc + 4 lb + 2 j)
    const int qr = (pr + p.pad_t) & 1, qc = (pc + p.pad_l) & 1;      // first tap row / column of the class

    f32x4 pf[FETCH];
    auto fetch = [&](int tile, int slice) {
        const int n = tile / (p.tiles_h * p.tiles_w), rem = tile - n * (p.tiles_h * p.tiles_w);
        const int th = rem / p.tiles_w, tw = rem - th * p.tiles_w;
        const int oh_lo = floor_half(th * TI + p.pad_t - 6), ow_lo = floor_half(tw * TI + p.pad_l - 6);
#pragma unroll
        for (int f = 0; f < FETCH; ++f) {
            const int i = f * 256 + tid;
            const int pix = i >> 2, c4 = (i & 3) * 4;
            const int rr = pix / TR, cc = pix - rr * TR;
            const int oh = oh_lo + rr, ow = ow_lo + cc;
            const bool ok = i < TR * TR * (CK / 4) && (unsigned)oh < (unsigned)p.OH && (unsigned)ow < (unsigned)p.OW;
            const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
            pf[f] = ok ? *reinterpret_cast<const f32x4 *>(p.dz + (((int64_t)n * p.OH + oh) * p.OW + ow) * p.ldx + slice * CK + c4) : zero;
        }
    };
    auto stage = [&]() {
#pragma unroll
        for (int f = 0; f < FETCH; ++f) {
            const int i = f * 256 + tid;
            if (i < TR * TR * (CK / 4)) *reinterpret_cast<f32x4 *>(dzl + (i >> 2) * PS + (i & 3) * 4) = pf[f];
        }
    };

    int tile = blockIdx.x;
    if (tile < p.tiles) fetch(tile, 0);
    for (; tile < p.tiles; tile += gridDim.x) {
        const int n = tile / (p.tiles_h * p.tiles_w), rem = tile - n * (p.tiles_h * p.tiles_w);
        const int th = rem / p.tiles_w, tw = rem - th * p.tiles_w;
        const int ih0 = th * TI, iw0 = tw * TI;
        // the lane's window: output row of its first pixel's last tap, relative to the staged rows (0 .. 19 with the 5 rows)
        const int oh_lo = floor_half(ih0 + p.pad_t - 6), ow_lo = floor_half(iw0 + p.pad_l - 6);
        const int er = (ih0 + pr + p.pad_t - qr) / 2 - oh_lo - 3, ec = (iw0 + pc + p.pad_l - qc) / 2 - ow_lo - 3;
        const int lane_off = ((er + 2 * la) * TR + ec + 2 * lb) * PS;
        Acc acc;
        const f32x2 z2 = {0.f, 0.f};
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) acc.a[i][j] = acc.b[i][j] = acc.e[i][j] = z2;
        for (int slice = 0; slice < NSLICE; ++slice) {
            __syncthreads();                  // (the previous slice is used up; the first pass: the filter is in LDS)
            stage();
            __syncthreads();
            const int ntile = tile + (int)gridDim.x;
            if (slice + 1 < NSLICE) fetch(tile, slice + 1);
            else if (ntile < p.tiles) fetch(ntile, 0);
            if (qr == 0 && qc == 0) class_slice<4, 4>(dzl, wl, lane_off, qr, qc, slice * CK, acc);
            else if (qr == 0) class_slice<4, 3>(dzl, wl, lane_off, qr, qc, slice * CK, acc);
            else if (qc == 0) class_slice<3, 4>(dzl, wl, lane_off, qr, qc, slice * CK, acc);
            else class_slice<3, 3>(dzl, wl, lane_off, qr, qc, slice * CK, acc);
        }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int ih = ih0 + pr + 4 * la + 2 * i, iw = iw0 + pc + 4 * lb + 2 * j;
                if (ih < p.H && iw < p.W) {
                    float *o = p.dx + (((int64_t)n * p.H + ih) * p.W + iw) * 3;
                    const f32x2 s = acc.a[i][j] + acc.b[i][j];
                    o[0] = s.x;
                    o[1] = s.y;
                    o[2] = acc.e[i][j].x + acc.e[i][j].y;
                }
            }
    }
}

int dgrad_grid(int64_t tiles) {
    const int64_t g = 2 * ds::kCUs;
    return (int)(tiles < g ? tiles : g);
}

}  // namespace

extern "C" int ds_conv_stem_dgrad_supported(int32_t H, int32_t W) { return H > 0 && W > 0 ? 1 : 0; }

extern "C" int ds_conv_stem_dgrad(const float *dz, const float *w, float *dx, int32_t N, int32_t H, int32_t W, int32_t cin_store,
                                  int32_t ldx, void *stream) {
    DS_REQUIRE(dz && w && dx, "ds_conv_stem_dgrad: null argument");
    DS_REQUIRE(N > 0 && ds_conv_stem_dgrad_supported(H, W), "ds_conv_stem_dgrad: geometry %d x %d x %d", N, H, W);
    DS_REQUIRE((cin_store == 3 || cin_store == 4) && ldx >= CO && ldx % 4 == 0 && (((uintptr_t)dz) & 15) == 0,
               "ds_conv_stem_dgrad: filter [7][7][3 or 4][64], dz with 16-byte aligned pixels of >= 64 channels");
    DgradParams p = {};
    p.dz = dz; p.w = w; p.dx = dx;
    p.N = N; p.H = H; p.W = W;
    p.OH = (H + 1) / 2; p.OW = (W + 1) / 2;
    const int ph = (p.OH - 1) * 2 + 7 - H, pw = (p.OW - 1) * 2 + 7 - W;     // TF SAME, as ds_conv_stem
    p.pad_t = (ph > 0 ? ph : 0) / 2; p.pad_l = (pw > 0 ? pw : 0) / 2;
    p.cin_store = cin_store; p.ldx = ldx;
    p.tiles_h = (H + TI - 1) / TI; p.tiles_w = (W + TI - 1) / TI;
    const int64_t tiles = (int64_t)N * p.tiles_h * p.tiles_w;
    DS_REQUIRE(tiles < (1ll << 31), "ds_conv_stem_dgrad: batch too large (split it)");
    p.tiles = (int)tiles;
    hipLaunchKernelGGL(conv_stem_dgrad_kernel, dim3(dgrad_grid(tiles)), dim3(256), 0, (hipStream_t)stream, p);
    return ds::check_launch("ds_conv_stem_dgrad");
}
