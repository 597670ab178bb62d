// The arithmetic of the JPEG reconstruction, ONE definition for the host function (jpeg_host.cpp, plain C++) and the
// device kernels (jpeg.hip): libjpeg's default decode path restated -- jpeg_idct_islow (CONST_BITS 13, PASS1_BITS 2),
// fancy h2v1 / h2v2 upsampling, the fixed-point ycc_rgb tables.  Integer arithmetic in 32 bits.  libjpeg-turbo's SIMD
// inverse DCT forms in0 + in4, in0 - in4, in7 + in3 and in5 + in1 in 16 bits in both passes and packs the pass-1 workspace
// with saturation; this statement is the same function only while no pass-1 output leaves +-16383, which the host entropy
// decoder guarantees per block (kColumnBound below: anything beyond is unsupported and decoded by the caller's
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

// ---- the Huffman decode of ONE restart segment ---------------------------------------------------------------------------------
// One definition for ds_jpeg_entropy_decode (jpeg_host.cpp), ds_jpeg_entropy_decode_segments_host and the device kernel
// (jpeg.hip).  A segment is byte-aligned and starts from zero DC predictors, so segments decode independently.  Every loop
// is bounded (a refill takes at most 8 bytes, a symbol at most 16 lengths, a block at most 64 symbols), every byte read is
// checked against the segment's end, and a failure is a DS_JPEG_E_* bit, never a guess.

#define DS_JPEG_ZIGZAG_INIT                                                                                                      \
    {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28, \
     35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63}

constexpr int kLookBits = 9;

// What keeps the reconstruction equal to libjpeg-turbo's SIMD jpeg_idct_islow, which forms in0 + in4, in0 - in4, in7 + in3 and
// in5 + in1 in 16 bits in BOTH passes and packs the pass-1 workspace with saturation: a block is taken only when no pass-1
// output can leave +-16383, so that nothing wraps or saturates there and the 32-bit statement above is the same function.
// A pass-1 output is 4 * sum_k w_k in_k over a column of dequantised coefficients with |w_0| = |w_4| = 1, |w_2|, |w_6| <=
// 1.30657 and |w_odd| <= 1.38704 (sqrt 2 cos); the test is sum_k ceil(4096 |w_k|) |in_k| <= 4090 * 4096 per column (4095.75
// less the rounding of the 13-bit constants and of the descale).  Pixel data cannot come near it: by Parseval a column of an
// 8-bit block has sum_k |w_k| |F_k| <= 3.62 * 1024.
constexpr int32_t kColumnBound = 4090 * 4096;
DS_HD int32_t row_weight(int row) { return (row & 1) ? 5682 : (row & 2) ? 5352 : 4096; }      // ceil(4096 |w_row|)

// the decoding tables of one DHT table
struct HuffTable {
    uint16_t look[1 << kLookBits]; // (length << 8) | symbol for codes of <= kLookBits bits, 0 otherwise
    int32_t maxcode[18];           // largest code of length l, -1 when none
    int32_t valoff[17];            // vals index of the first code of length l, minus that code
    uint8_t vals[256];
};

// derive the decoding tables from the DHT form (counts of the code lengths 1..16, then the values); false when the counts
// do not describe a prefix code of at most 256 values, or a DC table names a category beyond 15
DS_HD bool huff_build(const uint8_t *counts16, const uint8_t *values, bool dc, HuffTable &h) {
    int total = 0;
    for (int l = 0; l < 16; ++l) total += counts16[l];
    if (total > 256) return false;
    for (int i = 0; i < (1 << kLookBits); ++i) h.look[i] = 0;
    for (int i = 0; i < 256; ++i) h.vals[i] = i < total ? values[i] : 0;
    int32_t code = 0;
    int k = 0;
    h.valoff[0] = 0;
    h.maxcode[0] = -1;
    for (int l = 1; l <= 16; ++l) {
        const int count = counts16[l - 1];
        h.valoff[l] = k - code;
        if (count) {
            if (code + count > (1 << l)) return false;
            for (int i = 0; i < count; ++i, ++k, ++code) {
                if (l <= kLookBits) {
                    const int first = code << (kLookBits - l);
                    for (int j = 0; j < (1 << (kLookBits - l)); ++j) h.look[first + j] = (uint16_t)((l << 8) | h.vals[k]);
                }
            }
            h.maxcode[l] = code - 1;
        } else {
            h.maxcode[l] = -1;
        }
        code <<= 1;
    }
    h.maxcode[17] = 0x7fffffff;
    if (dc)
        for (int i = 0; i < total; ++i)
            if (h.vals[i] > 15) return false;
    return true;
}

// bits of one restart segment [p, end): inside it every 0xFF is followed by a stuffed 0x00 (the marker walk checked that);
// past its end the reader supplies zeros and counts them
struct Bits {
    const uint8_t *p, *end;
    uint64_t acc;
    int n;                         // bits in acc (from the top)
    int fake;                      // of which supplied past the end

    DS_HD void open(const uint8_t *begin, const uint8_t *stop) {
        p = begin;
        end = stop;
        acc = 0;
        n = fake = 0;
    }
    DS_HD void refill() {
        while (n <= 56) {
            if (p < end) {
                const uint8_t v = *p++;
                if (v == 0xFF && p < end) ++p;
                acc |= (uint64_t)v << (56 - n);
            } else {
                fake += 8;
            }
            n += 8;
        }
    }
    DS_HD uint32_t peek(int k) const { return (uint32_t)(acc >> (64 - k)); }
    DS_HD void skip(int k) {
        acc <<= k;
        n -= k;
    }
    DS_HD bool overrun() const { return n < fake; }
    // the segment is used up: every byte fetched, less than a byte of padding left, no bit taken from past its end
    DS_HD bool used_up() const { return p == end && !overrun() && n - fake < 8; }
};

// one Huffman symbol, -1 when no code matches; at least 16 bits are in the buffer
DS_HD int huff_decode(Bits &br, const HuffTable &h) {
    const uint16_t e = h.look[br.peek(kLookBits)];
    if (e) {
        br.skip(e >> 8);
        return e & 255;
    }
    for (int l = kLookBits + 1; l <= 16; ++l) {
        const int32_t code = (int32_t)br.peek(l);
        if (code <= h.maxcode[l]) {
            br.skip(l);
            return h.vals[(h.valoff[l] + code) & 255];
        }
    }
    return -1;
}

DS_HD int receive_extend(Bits &br, int s) {
    const int v = (int)br.peek(s);
    br.skip(s);
    return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
}

// One block into blk[0 .. 64) (natural order through `zigzag`; only non-zero coefficients and the DC are stored: the
// caller zeroed the storage).  q: the component's quantisers, for the checks.  column[0], column[stride], ..,
// column[7 * stride]: scratch for the weighted |dequantised coefficient| sums, at most 8 * 32767 * 5682 each (a lane of
// the kernel keeps them in LDS: a register array indexed at run time would go to scratch memory).  Returns 0 or one
// DS_JPEG_E_* bit.
DS_HD int decode_block(Bits &br, const HuffTable &dc, const HuffTable &ac, const uint8_t *q, const uint8_t *zigzag, int &pred,
                       int16_t *blk, int32_t *column, int stride) {
    br.refill();
    int s = huff_decode(br, dc);
    if (s < 0) return DS_JPEG_E_CODE;
    if (s) {
        br.refill();
        pred += receive_extend(br, s);
    }
    if (pred * (int)q[0] > 32767 || pred * (int)q[0] < -32767 || pred > 32767 || pred < -32767) return DS_JPEG_E_RANGE;
    blk[0] = (int16_t)pred;
    for (int c = 1; c < 8; ++c) column[c * stride] = 0;
    column[0] = row_weight(0) * (pred < 0 ? -pred : pred) * (int)q[0];
    for (int k = 1; k < 64;) {                     // k grows by at least one per turn
        br.refill();
        const int rs = huff_decode(br, ac);
        if (rs < 0) return DS_JPEG_E_CODE;
        const int r = rs >> 4;
        s = rs & 15;
        if (!s) {
            if (r != 15) break;                    // end of block
            k += 16;
            if (k > 64) return DS_JPEG_E_RUN;
            continue;
        }
        k += r;
        if (k > 63) return DS_JPEG_E_RUN;
        const int v = receive_extend(br, s);
        const int nat = zigzag[k];
        const int prod = v * (int)q[nat];
        if (prod > 32767 || prod < -32767) return DS_JPEG_E_RANGE;
        column[(nat & 7) * stride] += row_weight(nat >> 3) * (prod < 0 ? -prod : prod);
        blk[nat] = (int16_t)v;
        ++k;
    }
    for (int c = 0; c < 8; ++c)
        if (column[c * stride] > kColumnBound) return DS_JPEG_E_COLUMN;
    return br.overrun() ? DS_JPEG_E_SEGMENT : 0;
}

// what a segment decode reads besides the bytes: the tables and quantisers of each component (static indices only)
struct SegmentTables {
    const HuffTable *dc[3], *ac[3];
    const uint8_t *q[3];
    const uint8_t *zigzag;
};

// MCUs [first_mcu, first_mcu + mcus) of an image from the segment's bytes [begin, end), into the image's coefficient
// storage `coef` (zeroed by the caller).  The caller guarantees 0 <= first_mcu, first_mcu + mcus <= MCUs of `g`, so every
// store lies inside the image's g.blocks * 64 coefficients.  Returns 0 or one DS_JPEG_E_* bit.
DS_HD int decode_segment(const uint8_t *begin, const uint8_t *end, int64_t first_mcu, int64_t mcus, const Geometry &g,
                         const SegmentTables &t, int16_t *coef, int32_t *column, int stride) {
    Bits br;
    br.open(begin, end);
    int pred0 = 0, pred1 = 0, pred2 = 0;
    const int mw = g.bw[1];                        // MCUs per row (grey: bw[1] = bw[0])
    int my = (int)(first_mcu / mw), mx = (int)(first_mcu % mw);
    for (int64_t m = 0; m < mcus; ++m) {
        for (int v = 0; v < g.vs; ++v)             // (grey: hs = vs = 1)
            for (int h = 0; h < g.hs; ++h) {
                const int64_t blk = (int64_t)(my * g.vs + v) * g.bw[0] + (mx * g.hs + h);
                const int e = decode_block(br, *t.dc[0], *t.ac[0], t.q[0], t.zigzag, pred0, coef + blk * 64, column, stride);
                if (e) return e;
            }
        if (g.ncomp == 3) {
            const int64_t blk = (int64_t)my * mw + mx;
            int e = decode_block(br, *t.dc[1], *t.ac[1], t.q[1], t.zigzag, pred1, coef + (g.base[1] + blk) * 64, column, stride);
            if (e) return e;
            e = decode_block(br, *t.dc[2], *t.ac[2], t.q[2], t.zigzag, pred2, coef + (g.base[2] + blk) * 64, column, stride);
            if (e) return e;
        }
        if (++mx == mw) {
            mx = 0;
            ++my;
        }
    }
    return br.used_up() ? 0 : DS_JPEG_E_SEGMENT;
}

// the image record of a segment launch is usable: geometry, coefficient storage inside the buffer, segments inside the table
DS_HD bool scan_desc_ok(const ds_jpeg_scan_desc &d, int64_t ncoef, int64_t nsegs, Geometry &g) {
    if (!geometry(d.width, d.height, d.sampling, g)) return false;
    if (d.coef_offset < 0 || (d.coef_offset & 7) || d.coef_offset > ncoef || g.blocks * 64 > ncoef - d.coef_offset) return false;
    return d.first_segment >= 0 && d.segments >= 1 && d.first_segment <= nsegs && d.segments <= nsegs - d.first_segment;
}

// segment i of an image (prev: segment i - 1, ignored for i = 0) lies inside the scan bytes and continues the MCU sequence
DS_HD bool segment_ok(const ds_jpeg_segment &s, const ds_jpeg_segment &prev, int i, int count, int64_t nscan, int64_t image_mcus) {
    if (s.begin < 0 || s.begin > s.end || s.end > nscan || s.first_mcu < 0 || s.mcus < 1) return false;
    if ((int64_t)s.first_mcu + s.mcus > image_mcus) return false;
    if (s.first_mcu != (i ? (int64_t)prev.first_mcu + prev.mcus : 0)) return false;
    return i + 1 < count || (int64_t)s.first_mcu + s.mcus == image_mcus;
}

DS_HD int64_t mcu_count(const Geometry &g) { return (int64_t)g.bw[1] * g.bh[1]; }      // (grey: the chroma grid equals the luma grid)

}  // namespace dsjpeg
