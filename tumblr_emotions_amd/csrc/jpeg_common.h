// The arithmetic of the JPEG reconstruction, ONE definition for the host function (jpeg_host.cpp, plain C++) and the
// device kernels (jpeg.hip): libjpeg's default decode path restated -- jpeg_idct_islow (CONST_BITS 13, PASS1_BITS 2),
// fancy h2v1 / h2v2 upsampling, the fixed-point ycc_rgb tables.  Integer arithmetic in 32 bits.  libjpeg-turbo's SIMD
// inverse DCT forms in0 + in4, in0 - in4, in7 + in3 and in5 + in1 in 16 bits in both passes and packs the pass-1 workspace
// with saturation; this statement is the same function only while no pass-1 output leaves +-16383, which the host entropy
// decoder guarantees per block (jpeg_host.cpp, kColumnBound: anything beyond is unsupported and decoded by the caller's
// other path).  Sums are formed in uint32_t and pass 1 clamps to int16 all the same, so that coefficients from any other
// source wrap or clamp instead of overflowing; the sample is clamped to 0..255.
#pragma once
#include <stdint.h>
#include "ds_kernels.h"

#if defined(__HIPCC__)
#define DS_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define DS_HD inline
#endif

namespace dsjpeg {

// block grid of a sampling class: luma h x v, MCU = (8 h) x (8 v) pixels
struct Geometry {
    int ncomp, hs, vs;
    int bw[3], bh[3];          // padded block grid per component
    int dw, dh;                // chroma downsampled_width / _height (= width, height when not subsampled)
    int64_t base[3];           // first block of the component in the image's storage
    int64_t blocks;            // all components
};

DS_HD bool geometry(int width, int height, int sampling, Geometry &g) {
    if (width < 1 || height < 1 || width > 65535 || height > 65535 || sampling < DS_JPEG_444 || sampling > DS_JPEG_GREY)
        return false;
    g.ncomp = sampling == DS_JPEG_GREY ? 1 : 3;
    g.hs = sampling == DS_JPEG_422 || sampling == DS_JPEG_420 ? 2 : 1;
    g.vs = sampling == DS_JPEG_420 ? 2 : 1;
    const int mx = (width + 8 * g.hs - 1) / (8 * g.hs), my = (height + 8 * g.vs - 1) / (8 * g.vs);
    g.bw[0] = mx * g.hs;
    g.bh[0] = my * g.vs;
    g.bw[1] = g.bw[2] = mx;
    g.bh[1] = g.bh[2] = my;
    g.dw = (width + g.hs - 1) / g.hs;
    g.dh = (height + g.vs - 1) / g.vs;
    g.base[0] = 0;
    g.base[1] = (int64_t)g.bw[0] * g.bh[0];
    g.base[2] = g.base[1] + (int64_t)mx * my;
    g.blocks = g.ncomp == 1 ? g.base[1] : g.base[2] + (int64_t)mx * my;
    return true;
}

DS_HD int32_t descale(uint32_t x, int n) { return (int32_t)(x + (1u << (n - 1))) >> n; }

// one 1-D pass of jpeg_idct_islow: in[0..7] -> out[0..7], descaled by `shift` bits
DS_HD void idct_1d(const int32_t in[8], int32_t out[8], int shift) {
    const uint32_t i0 = (uint32_t)in[0], i1 = (uint32_t)in[1], i2 = (uint32_t)in[2], i3 = (uint32_t)in[3];
    const uint32_t i4 = (uint32_t)in[4], i5 = (uint32_t)in[5], i6 = (uint32_t)in[6], i7 = (uint32_t)in[7];
    // even part
    uint32_t z1 = (i2 + i6) * 4433u;                       // FIX_0_541196100
    const uint32_t e2 = z1 - i6 * 15137u;                  // FIX_1_847759065
    const uint32_t e3 = z1 + i2 * 6270u;                   // FIX_0_765366865
    const uint32_t e0 = (i0 + i4) << 13, e1 = (i0 - i4) << 13;
    const uint32_t t10 = e0 + e3, t13 = e0 - e3, t11 = e1 + e2, t12 = e1 - e2;
    // odd part
    uint32_t o0 = i7, o1 = i5, o2 = i3, o3 = i1;
    z1 = o0 + o3;
    uint32_t z2 = o1 + o2, z3 = o0 + o2, z4 = o1 + o3;
    const uint32_t z5 = (z3 + z4) * 9633u;                 // FIX_1_175875602
    o0 *= 2446u;                                           // FIX_0_298631336
    o1 *= 16819u;                                          // FIX_2_053119869
    o2 *= 25172u;                                          // FIX_3_072711026
    o3 *= 12299u;                                          // FIX_1_501321110
    z1 *= (uint32_t)-7373;                                 // -FIX_0_899976223
    z2 *= (uint32_t)-20995;                                // -FIX_2_562915447
    z3 *= (uint32_t)-16069;                                // -FIX_1_961570560
    z4 *= (uint32_t)-3196;                                 // -FIX_0_390180644
    z3 += z5;
    z4 += z5;
    o0 += z1 + z3;
    o1 += z2 + z4;
    o2 += z2 + z3;
    o3 += z1 + z4;
    out[0] = descale(t10 + o3, shift);
    out[7] = descale(t10 - o3, shift);
    out[1] = descale(t11 + o2, shift);
    out[6] = descale(t11 - o2, shift);
    out[2] = descale(t12 + o1, shift);
    out[5] = descale(t12 - o1, shift);
    out[3] = descale(t13 + o0, shift);
    out[4] = descale(t13 - o0, shift);
}

DS_HD int32_t sat16(int32_t v) { return v < -32768 ? -32768 : v > 32767 ? 32767 : v; }
DS_HD int32_t sat8(int32_t v) { return v < 0 ? 0 : v > 255 ? 255 : v; }

// pass 1 (a column): dequantised inputs, CONST_BITS - PASS1_BITS = 11, int16 workspace
DS_HD void idct_column(const int32_t in[8], int32_t out[8]) {
    idct_1d(in, out, 11);
    for (int k = 0; k < 8; ++k) out[k] = sat16(out[k]);
}

// pass 2 (a row): CONST_BITS + PASS1_BITS + 3 = 18, + 128, 0..255
DS_HD void idct_row(const int32_t in[8], int32_t out[8]) {
    idct_1d(in, out, 18);
    for (int k = 0; k < 8; ++k) out[k] = sat8(out[k] + 128);
}

// a component plane: uint8 samples, `pitch` bytes per row
struct Plane {
    const uint8_t *p;
    int pitch;
};
DS_HD int at(const Plane &pl, int y, int x) { return pl.p[(int64_t)y * pl.pitch + x]; }

// the chroma sample libjpeg's upsampler puts at pixel (y, x): fancy when downsampled_width > 2, replication otherwise
DS_HD int chroma(const Plane &pl, const Geometry &g, int y, int x) {
    if (g.hs == 1) return at(pl, y, x);
    const int i = x >> 1;
    if (g.dw <= 2) return at(pl, g.vs == 2 ? y >> 1 : y, i);
    if (g.vs == 1) {                                         // h2v1
        const int s = at(pl, y, i);
        if (x & 1) return i == g.dw - 1 ? s : (3 * s + at(pl, y, i + 1) + 2) >> 2;
        return i == 0 ? s : (3 * s + at(pl, y, i - 1) + 1) >> 2;
    }
    // h2v2: the nearer chroma row weighs 3, the farther 1; at the top and the bottom the farther row is the edge row itself
    const int r = y >> 1;
    int far = (y & 1) ? r + 1 : r - 1;
    far = far < 0 ? 0 : far > g.dh - 1 ? g.dh - 1 : far;
    const int cur = 3 * at(pl, r, i) + at(pl, far, i);
    if (x & 1) {
        if (i == g.dw - 1) return (4 * cur + 7) >> 4;
        return (3 * cur + 3 * at(pl, r, i + 1) + at(pl, far, i + 1) + 7) >> 4;
    }
    if (i == 0) return (4 * cur + 8) >> 4;
    return (3 * cur + 3 * at(pl, r, i - 1) + at(pl, far, i - 1) + 8) >> 4;
}

constexpr int32_t fix(double x) { return (int32_t)(x * 65536.0 + 0.5); }

// ycc_rgb_convert through its tables' expressions
DS_HD void ycc_to_rgb(int y, int cb, int cr, uint8_t rgb[3]) {
    cb -= 128;
    cr -= 128;
    rgb[0] = (uint8_t)sat8(y + ((fix(1.40200) * cr + 32768) >> 16));
    rgb[1] = (uint8_t)sat8(y + ((-fix(0.34414) * cb + 32768 - fix(0.71414) * cr) >> 16));
    rgb[2] = (uint8_t)sat8(y + ((fix(1.77200) * cb + 32768) >> 16));
}

// pixel (y, x) of the decoded image from the three (or one) component planes
DS_HD void pixel(const Plane pl[3], const Geometry &g, int y, int x, uint8_t rgb[3]) {
    const int lum = at(pl[0], y, x);
    if (g.ncomp == 1) {
        rgb[0] = rgb[1] = rgb[2] = (uint8_t)lum;
        return;
    }
    ycc_to_rgb(lum, chroma(pl[1], g, y, x), chroma(pl[2], g, y, x), rgb);
}

// the planes of an image inside a byte buffer laid out like its coefficient storage
DS_HD void planes_of(const uint8_t *base, const Geometry &g, Plane pl[3]) {
    for (int c = 0; c < 3; ++c) {
        pl[c].p = base + (c < g.ncomp ? g.base[c] * 64 : 0);
        pl[c].pitch = g.bw[c < g.ncomp ? c : 0] * 8;
    }
}

}  // namespace dsjpeg
