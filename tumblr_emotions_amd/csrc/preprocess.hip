// Image preprocessing on the device (ds_preprocess_eval; ds_preprocess_train further down).  Eval time: the arithmetic of preprocess_for_eval
// (slim/preprocessing/inception_preprocessing.py:237-275 as called by image_model/im_model.py:78-116) for a ragged batch
// of decoded, already centrally cropped uint8 RGB images:
//   convert_image_dtype (v / 255, through a 256-entry table)  ->  TF-1 legacy bilinear resize  ->  (x - 0.5) * 2
// Bit-identical to the NumPy path: every operation is a single fp32 rounding in NumPy's order, so the kernel body is
// compiled with fp contraction OFF (a + (b - a) * f as v_mul_f32 + v_add_f32, never v_fmac_f32).  The crop geometry and
// the two scales are computed on the host in Python doubles; nothing here replicates double arithmetic.
//
// Shape: a bandwidth kernel.  A workgroup owns one output row at a time (grid-stride over batch x out_h rows): the two
// source rows of that output row are staged into LDS with aligned dword loads (rows of a ragged byte buffer start at
// any byte), the out_w * 3 floats of the row are then produced from LDS byte reads and stored as one contiguous
// stream, consecutive lanes on consecutive floats.  One writer per element, no atomics.  Source rows wider than the LDS
// window (more than kRowBytes bytes, i.e. beyond 4095 pixels) are gathered from global memory instead.
#include "ds_common.h"

namespace {

constexpr int kRowBytes = 12288;            // LDS window per source row (two rows per workgroup: 24 KB, 6 workgroups / CU)
constexpr int kRowWords = kRowBytes / 4;

// the aligned dword at byte address `a` of the buffer (a % 4 == 0); the last dword may straddle the end of the buffer
__device__ __forceinline__ uint32_t load_word(const uint8_t *bytes, int64_t nbytes, int64_t a) {
    if (a + 4 <= nbytes) return *reinterpret_cast<const uint32_t *>(bytes + a);
    uint32_t v = 0;
    for (int k = 0; k < 4; ++k)
        if (a + k < nbytes) v |= (uint32_t)bytes[a + k] << (8 * k);
    return v;
}

__global__ __launch_bounds__(256) void preprocess_eval_kernel(const uint8_t *__restrict__ bytes, int64_t nbytes,
                                                              const ds_preprocess_desc *__restrict__ desc, int batch,
                                                              const float *__restrict__ lut, float *__restrict__ out,
                                                              int out_h, int out_w) {
#pragma clang fp contract(off)
    __shared__ uint32_t rows[2][kRowWords];
    __shared__ float table[256];
    table[threadIdx.x] = lut[threadIdx.x];
    const int total_rows = batch * out_h;          // < 2^31: checked by the host entry point
    const int row_floats = out_w * 3;
    for (int r = blockIdx.x; r < total_rows; r += gridDim.x) {
        const int b = r / out_h, oy = r - b * out_h;
        const ds_preprocess_desc d = desc[b];
        const int h = d.height, w = d.width;
        const float sy = (float)oy * d.scale_y;
        const float fy0 = floorf(sy);
        int y0 = (int)fy0;
        y0 = y0 < h - 1 ? y0 : h - 1;
        const int y1 = y0 + 1 < h - 1 ? y0 + 1 : h - 1;
        const float fy = sy - fy0;
        const int64_t pitch = (int64_t)w * 3;
        const int64_t s0 = d.offset + y0 * pitch, s1 = d.offset + y1 * pitch;      // first byte of the two source rows
        const int64_t a0 = s0 & ~(int64_t)3, a1 = s1 & ~(int64_t)3;
        const bool staged = pitch + 3 <= kRowBytes;                                // wave-uniform (whole workgroup)
        __syncthreads();                                                           // previous row's readers are done (and: table)
        if (staged) {
            const int n0 = (int)((s0 + pitch - a0 + 3) >> 2), n1 = (int)((s1 + pitch - a1 + 3) >> 2);
            for (int i = threadIdx.x; i < n0; i += 256) rows[0][i] = load_word(bytes, nbytes, a0 + 4 * (int64_t)i);
            for (int i = threadIdx.x; i < n1; i += 256) rows[1][i] = load_word(bytes, nbytes, a1 + 4 * (int64_t)i);
        }
        __syncthreads();
        const uint8_t *p0 = staged ? reinterpret_cast<const uint8_t *>(rows[0]) + (int)(s0 - a0) : bytes + s0;
        const uint8_t *p1 = staged ? reinterpret_cast<const uint8_t *>(rows[1]) + (int)(s1 - a1) : bytes + s1;
        float *dst = out + (int64_t)r * row_floats;
        for (int e = threadIdx.x; e < row_floats; e += 256) {
            const int ox = e / 3, c = e - ox * 3;
            const float sx = (float)ox * d.scale_x;
            const float fx0 = floorf(sx);
            int x0 = (int)fx0;
            x0 = x0 < w - 1 ? x0 : w - 1;
            const int x1 = x0 + 1 < w - 1 ? x0 + 1 : w - 1;
            const float fx = sx - fx0;
            const float tl = table[p0[x0 * 3 + c]], tr = table[p0[x1 * 3 + c]];
            const float bl = table[p1[x0 * 3 + c]], br = table[p1[x1 * 3 + c]];
            const float top = tl + (tr - tl) * fx;
            const float bot = bl + (br - bl) * fx;
            const float v = top + (bot - top) * fy;
            dst[e] = (v - 0.5f) * 2.0f;
        }
    }
}


// ---- train-time sibling: preprocess_for_train (slim/preprocessing/inception_preprocessing.py:156-234, fast mode) ---------------
// The host has drawn every random choice and sliced the sampled crop; per output PIXEL (HSV needs the three channels
// together) a lane does: table lookup, the two-axis bilinear blend at the mirrored column when the image is flipped,
// brightness / saturation in the image's order, clip to [0, 1], (x - 0.5) * 2 -- each operation one fp32 rounding in the
// order of the NumPy definition (preprocessing/inception_preprocessing.py: adjust_saturation, distort_color_fast); the two
// divisions are IEEE divisions (v_div_scale / v_div_fmas / v_div_fixup: no fast-math flag is passed to this file).
// Same staging as the eval kernel.  A lane owns the 12 output bytes of its pixel and stores them as one global_store_dwordx3:
// the 64 lanes of a wave cover 768 contiguous bytes with one instruction, so every cache line is written whole by one wave.
static_assert(sizeof(ds_preprocess_train_desc) == 40 && offsetof(ds_preprocess_train_desc, offset) == 0 &&
                  offsetof(ds_preprocess_train_desc, height) == 8 && offsetof(ds_preprocess_train_desc, width) == 12 &&
                  offsetof(ds_preprocess_train_desc, scale_y) == 16 && offsetof(ds_preprocess_train_desc, scale_x) == 20 &&
                  offsetof(ds_preprocess_train_desc, delta) == 24 && offsetof(ds_preprocess_train_desc, factor) == 28 &&
                  offsetof(ds_preprocess_train_desc, flags) == 32 && offsetof(ds_preprocess_train_desc, reserved) == 36,
              "ds_preprocess_train_desc is ABI: ops.preprocess_train_desc_dtype() mirrors this layout");

struct __attribute__((packed, aligned(4))) rgb_f32 {
    float r, g, b;
};

// AdjustSaturation on one pixel, in place
__device__ __forceinline__ void saturate_pixel(float &r, float &g, float &b, float factor) {
#pragma clang fp contract(off)
    const float v = fmaxf(fmaxf(r, g), b);
    const float mn = fminf(fminf(r, g), b);
    const float range = v - mn;
    float s = v > 0.0f ? range / v : 0.0f;
    const float norm = 1.0f / (range > 0.0f ? 6.0f * range : 1.0f);
    float h = r == v ? norm * (g - b) : g == v ? norm * (b - r) + (float)(2.0 / 6.0) : norm * (r - g) + (float)(4.0 / 6.0);
    if (range <= 0.0f) h = 0.0f;
    if (h < 0.0f) h = h + 1.0f;
    s = fminf(1.0f, fmaxf(0.0f, s * factor));
    const float c = s * v;
    const float m = v - c;
    const float dh = h * 6.0f;
    const int cat = (int)dh;
    float f = dh;
    while (f <= 0.0f) f = f + 2.0f;
    while (f >= 2.0f) f = f - 2.0f;
    const float x = c * (1.0f - fabsf(f - 1.0f));
    float rr = 0.0f, gg = 0.0f, bb = 0.0f;
    switch (cat) {
        case 0: rr = c; gg = x; break;
        case 1: rr = x; gg = c; break;
        case 2: gg = c; bb = x; break;
        case 3: gg = x; bb = c; break;
        case 4: rr = x; bb = c; break;
        case 5: rr = c; bb = x; break;
        default: break;
    }
    r = rr + m;
    g = gg + m;
    b = bb + m;
}

__global__ __launch_bounds__(256) void preprocess_train_kernel(const uint8_t *__restrict__ bytes, int64_t nbytes,
                                                               const ds_preprocess_train_desc *__restrict__ desc, int batch,
                                                               const float *__restrict__ lut, float *__restrict__ out,
                                                               int out_h, int out_w) {
#pragma clang fp contract(off)
    __shared__ uint32_t rows[2][kRowWords];
    __shared__ float table[256];
    table[threadIdx.x] = lut[threadIdx.x];
    const int total_rows = batch * out_h;          // < 2^31: checked by the host entry point
    for (int r = blockIdx.x; r < total_rows; r += gridDim.x) {
        const int b = r / out_h, oy = r - b * out_h;
        const ds_preprocess_train_desc d = desc[b];
        const int h = d.height, w = d.width;
        const bool flip = (d.flags & DS_PREPROCESS_FLIP) != 0, sat_first = (d.flags & DS_PREPROCESS_SATURATION_FIRST) != 0;
        const float sy = (float)oy * d.scale_y;
        const float fy0 = floorf(sy);
        int y0 = (int)fy0;
        y0 = y0 < h - 1 ? y0 : h - 1;
        const int y1 = y0 + 1 < h - 1 ? y0 + 1 : h - 1;
        const float fy = sy - fy0;
        const int64_t pitch = (int64_t)w * 3;
        const int64_t s0 = d.offset + y0 * pitch, s1 = d.offset + y1 * pitch;      // first byte of the two source rows
        const int64_t a0 = s0 & ~(int64_t)3, a1 = s1 & ~(int64_t)3;
        const bool staged = pitch + 3 <= kRowBytes;                                // wave-uniform (whole workgroup)
        __syncthreads();                                                           // previous row's readers are done (and: table)
        if (staged) {
            const int n0 = (int)((s0 + pitch - a0 + 3) >> 2), n1 = (int)((s1 + pitch - a1 + 3) >> 2);
            for (int i = threadIdx.x; i < n0; i += 256) rows[0][i] = load_word(bytes, nbytes, a0 + 4 * (int64_t)i);
            for (int i = threadIdx.x; i < n1; i += 256) rows[1][i] = load_word(bytes, nbytes, a1 + 4 * (int64_t)i);
        }
        __syncthreads();
        const uint8_t *p0 = staged ? reinterpret_cast<const uint8_t *>(rows[0]) + (int)(s0 - a0) : bytes + s0;
        const uint8_t *p1 = staged ? reinterpret_cast<const uint8_t *>(rows[1]) + (int)(s1 - a1) : bytes + s1;
        rgb_f32 *dst = reinterpret_cast<rgb_f32 *>(out + (int64_t)r * out_w * 3);
        for (int ox = threadIdx.x; ox < out_w; ox += 256) {
            const int rx = flip ? out_w - 1 - ox : ox;                             // column of the resized, unflipped image
            const float sx = (float)rx * d.scale_x;
            const float fx0 = floorf(sx);
            int x0 = (int)fx0;
            x0 = x0 < w - 1 ? x0 : w - 1;
            const int x1 = x0 + 1 < w - 1 ? x0 + 1 : w - 1;
            const float fx = sx - fx0;
            float px[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float tl = table[p0[x0 * 3 + c]], tr = table[p0[x1 * 3 + c]];
                const float bl = table[p1[x0 * 3 + c]], br = table[p1[x1 * 3 + c]];
                const float top = tl + (tr - tl) * fx;
                const float bot = bl + (br - bl) * fx;
                px[c] = top + (bot - top) * fy;
            }
            if (!sat_first) {
                px[0] = px[0] + d.delta;
                px[1] = px[1] + d.delta;
                px[2] = px[2] + d.delta;
            }
            saturate_pixel(px[0], px[1], px[2], d.factor);
            if (sat_first) {
                px[0] = px[0] + d.delta;
                px[1] = px[1] + d.delta;
                px[2] = px[2] + d.delta;
            }
            rgb_f32 o;
            o.r = (fminf(fmaxf(px[0], 0.0f), 1.0f) - 0.5f) * 2.0f;
            o.g = (fminf(fmaxf(px[1], 0.0f), 1.0f) - 0.5f) * 2.0f;
            o.b = (fminf(fmaxf(px[2], 0.0f), 1.0f) - 0.5f) * 2.0f;
            dst[ox] = o;
        }
    }
}

}  // namespace

extern "C" int ds_preprocess_eval(const uint8_t *bytes, int64_t nbytes, const ds_preprocess_desc *desc, int32_t batch,
                                  const float *lut, float *out, int32_t out_h, int32_t out_w, void *stream) {
    DS_REQUIRE(bytes && desc && lut && out && nbytes > 0 && batch > 0 && out_h > 0 && out_w > 0,
               "ds_preprocess_eval: bad argument");
    DS_REQUIRE(((uintptr_t)bytes & 3) == 0, "ds_preprocess_eval: the byte buffer must be 4-byte aligned");
    DS_REQUIRE((int64_t)batch * out_h < (1ll << 31) - ds::kMaxStreamBlocks && out_w < (1 << 29), "ds_preprocess_eval: batch x out_h too large");
    const int grid = ds::stream_grid((int64_t)batch * out_h, 1);
    hipLaunchKernelGGL(preprocess_eval_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, bytes, nbytes, desc, (int)batch,
                       lut, out, (int)out_h, (int)out_w);
    return ds::check_launch("ds_preprocess_eval");
}

extern "C" int ds_preprocess_train(const uint8_t *bytes, int64_t nbytes, const ds_preprocess_train_desc *desc, int32_t batch,
                                   const float *lut, float *out, int32_t out_h, int32_t out_w, void *stream) {
    DS_REQUIRE(bytes && desc && lut && out && nbytes > 0 && batch > 0 && out_h > 0 && out_w > 0,
               "ds_preprocess_train: bad argument");
    DS_REQUIRE(((uintptr_t)bytes & 3) == 0, "ds_preprocess_train: the byte buffer must be 4-byte aligned");
    DS_REQUIRE(((uintptr_t)out & 3) == 0, "ds_preprocess_train: the output must be 4-byte aligned");
    DS_REQUIRE((int64_t)batch * out_h < (1ll << 31) - ds::kMaxStreamBlocks && out_w < (1 << 29), "ds_preprocess_train: batch x out_h too large");
    const int grid = ds::stream_grid((int64_t)batch * out_h, 1);
    hipLaunchKernelGGL(preprocess_train_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, bytes, nbytes, desc, (int)batch,
                       lut, out, (int)out_h, (int)out_w);
    return ds::check_launch("ds_preprocess_train");
}
