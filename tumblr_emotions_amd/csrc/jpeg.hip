// The device side of the baseline JPEG decode.  ds_jpeg_entropy_decode_device (opt-in, restart-segmented streams only) is at
// the end of the file.  The parallel half of the decode (ds_jpeg_reconstruct): quantised coefficients -> the ragged uint8 RGB crops
// that ds_preprocess_eval / ds_preprocess_train read.  The arithmetic is jpeg_common.h's (shared with the host statement in
// jpeg_host.cpp): integers only, so the bytes equal libjpeg's.  Two launches, blockIdx.y = image:
//
//   jpeg_idct_kernel      dequantise + jpeg_idct_islow of the blocks that intersect the crop plus a one-sample chroma halo
//                         (what the upsampler reads), into uint8 component planes in scratch.  A workgroup takes 32 blocks
//                         at a time: lane (block, row) stages one 16-byte coefficient row into LDS; lane (block, column)
//                         runs pass 1 down its column; lane (row, block) runs pass 2 along its row and stores its 8 samples
//                         as one 8-byte word -- 32 consecutive lanes write 256 contiguous bytes of a plane row when the
//                         blocks are neighbours.  No zero-coefficient shortcut: every lane runs the same 16 multiplies per
//                         pass whatever the image holds.  The image's quantisation tables sit in LDS.  LDS rows are padded
//                         (72 instead of 64 entries) so that the four blocks of a half-wave fall on different banks.
//   jpeg_colour_kernel    upsample + YCbCr -> RGB + crop: a lane owns 4 consecutive pixels of the crop = 12 bytes = three
//                         aligned dwords (the crop starts on a 4-byte boundary), stored as one global_store_dwordx3; the
//                         last, partial group of an image is stored bytewise.  Exactly one lane writes each byte.
#include "ds_common.h"
#include "jpeg_common.h"

namespace {

static_assert(sizeof(ds_jpeg_desc) == 240 && offsetof(ds_jpeg_desc, coef_offset) == 0 && offsetof(ds_jpeg_desc, out_offset) == 8 &&
                  offsetof(ds_jpeg_desc, width) == 16 && offsetof(ds_jpeg_desc, sampling) == 24 && offsetof(ds_jpeg_desc, y0) == 28 &&
                  offsetof(ds_jpeg_desc, crop_w) == 40 && offsetof(ds_jpeg_desc, quant) == 48,
              "ds_jpeg_desc is ABI: ops.jpeg_desc_dtype() mirrors this layout");

constexpr int kUnits = 32;                 // blocks per workgroup iteration (8 lanes each)
constexpr int kPad = 72;                   // padded LDS row of a block

// the descriptor is usable: geometry, crop inside the image, storage inside the buffers (uniform over the workgroup)
__device__ __forceinline__ bool usable(const ds_jpeg_desc &d, int64_t ncoef, int64_t nbytes, int64_t scratch_bytes,
                                       dsjpeg::Geometry &g) {
    if (!dsjpeg::geometry(d.width, d.height, d.sampling, g)) return false;
    if (d.y0 < 0 || d.x0 < 0 || d.crop_h < 1 || d.crop_w < 1 || d.crop_h > d.height - d.y0 || d.crop_w > d.width - d.x0) return false;
    if (d.coef_offset < 0 || (d.coef_offset & 7) || d.coef_offset > ncoef || g.blocks * 64 > ncoef - d.coef_offset) return false;
    if (d.coef_offset + g.blocks * 64 > scratch_bytes) return false;
    const int64_t out_n = (int64_t)d.crop_h * d.crop_w * 3;
    return d.out_offset >= 0 && !(d.out_offset & 3) && d.out_offset <= nbytes && out_n <= nbytes - d.out_offset;
}

__global__ __launch_bounds__(256) void jpeg_idct_kernel(const int16_t *__restrict__ coef, int64_t ncoef,
                                                        const ds_jpeg_desc *__restrict__ desc, int64_t nbytes,
                                                        uint8_t *__restrict__ scratch, int64_t scratch_bytes) {
    __shared__ __attribute__((aligned(16))) int16_t s_coef[kUnits][kPad];
    __shared__ __attribute__((aligned(16))) int32_t s_ws[kUnits][kPad];
    __shared__ int32_t s_q[3][64];
    __shared__ int64_t s_src[kUnits];      // first coefficient of the unit's block, -1 = no unit
    __shared__ int64_t s_dst[kUnits];      // first byte of the block in its plane
    __shared__ int32_t s_meta[kUnits];     // component | plane pitch << 2

    const ds_jpeg_desc &d = desc[blockIdx.y];
    dsjpeg::Geometry g;
    if (!usable(d, ncoef, nbytes, scratch_bytes, g)) return;
    const int t = threadIdx.x;
    if (t < 192) s_q[t >> 6][t & 63] = d.quant[t >> 6][t & 63];

    // block ranges per component: the crop, widened by one chroma sample where the component is upsampled
    int bx0[3], by0[3], nbx[3], start[4];
    start[0] = 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        int xa = d.x0, xb = d.x0 + d.crop_w - 1, ya = d.y0, yb = d.y0 + d.crop_h - 1;
        if (c > 0 && g.hs == 2) {
            xa = (xa >> 1) - 1 < 0 ? 0 : (xa >> 1) - 1;
            xb = (xb >> 1) + 1 > g.dw - 1 ? g.dw - 1 : (xb >> 1) + 1;
        }
        if (c > 0 && g.vs == 2) {
            ya = (ya >> 1) - 1 < 0 ? 0 : (ya >> 1) - 1;
            yb = (yb >> 1) + 1 > g.dh - 1 ? g.dh - 1 : (yb >> 1) + 1;
        }
        bx0[c] = xa >> 3;
        by0[c] = ya >> 3;
        nbx[c] = (xb >> 3) - bx0[c] + 1;
        start[c + 1] = start[c] + (c < g.ncomp ? nbx[c] * ((yb >> 3) - by0[c] + 1) : 0);
    }
    const int total = start[3];

    for (int first = blockIdx.x * kUnits; first < total; first += gridDim.x * kUnits) {
        __syncthreads();                                   // the previous iteration's readers are done (and: s_q)
        if (t < kUnits) {
            const int u = first + t;
            int64_t src = -1, dst = 0;
            int meta = 0;
            if (u < total) {
                const int c = u < start[1] ? 0 : u < start[2] ? 1 : 2;      // selects, not indexing: the tables stay in registers
                const int local = u - (c == 0 ? 0 : c == 1 ? start[1] : start[2]);
                const int nx = c == 0 ? nbx[0] : c == 1 ? nbx[1] : nbx[2];
                const int by = (c == 0 ? by0[0] : c == 1 ? by0[1] : by0[2]) + local / nx;
                const int bx = (c == 0 ? bx0[0] : c == 1 ? bx0[1] : bx0[2]) + local % nx;
                const int bwc = c == 0 ? g.bw[0] : g.bw[1];
                const int64_t basec = c == 0 ? 0 : c == 1 ? g.base[1] : g.base[2];
                const int pitch = bwc * 8;
                src = d.coef_offset + (basec + (int64_t)by * bwc + bx) * 64;
                dst = d.coef_offset + basec * 64 + (int64_t)by * 8 * pitch + bx * 8;
                meta = c | (pitch << 2);
            }
            s_src[t] = src;
            s_dst[t] = dst;
            s_meta[t] = meta;
        }
        __syncthreads();
        {   // stage: lane (block, row) moves one 16-byte row
            const int u = t >> 3, j = t & 7;
            const int64_t src = s_src[u];
            uint4 v = make_uint4(0, 0, 0, 0);
            if (src >= 0) v = *reinterpret_cast<const uint4 *>(coef + src + j * 8);
            *reinterpret_cast<uint4 *>(&s_coef[u][j * 8]) = v;
        }
        __syncthreads();
        {   // pass 1: lane (block, column)
            const int u = t >> 3, j = t & 7;
            const int c = s_meta[u] & 3;
            int32_t in[8], out[8];
#pragma unroll
            for (int r = 0; r < 8; ++r) in[r] = (int32_t)s_coef[u][r * 8 + j] * s_q[c][r * 8 + j];
            dsjpeg::idct_column(in, out);
#pragma unroll
            for (int r = 0; r < 8; ++r) s_ws[u][r * 8 + j] = out[r];
        }
        __syncthreads();
        {   // pass 2: lane (row, block)
            const int u = t & 31, r = t >> 5;
            int32_t in[8], out[8];
            const int4 lo = *reinterpret_cast<const int4 *>(&s_ws[u][r * 8]), hi = *reinterpret_cast<const int4 *>(&s_ws[u][r * 8 + 4]);
            in[0] = lo.x, in[1] = lo.y, in[2] = lo.z, in[3] = lo.w, in[4] = hi.x, in[5] = hi.y, in[6] = hi.z, in[7] = hi.w;
            dsjpeg::idct_row(in, out);
            if (s_src[u] >= 0) {
                uint2 w;
                w.x = (uint32_t)out[0] | (uint32_t)out[1] << 8 | (uint32_t)out[2] << 16 | (uint32_t)out[3] << 24;
                w.y = (uint32_t)out[4] | (uint32_t)out[5] << 8 | (uint32_t)out[6] << 16 | (uint32_t)out[7] << 24;
                *reinterpret_cast<uint2 *>(scratch + s_dst[u] + (int64_t)r * (s_meta[u] >> 2)) = w;
            }
        }
    }
}

struct __attribute__((packed, aligned(4))) rgb4 {
    uint32_t a, b, c;
};

__global__ __launch_bounds__(256) void jpeg_colour_kernel(const uint8_t *__restrict__ scratch, int64_t scratch_bytes,
                                                          const ds_jpeg_desc *__restrict__ desc, int64_t ncoef,
                                                          uint8_t *__restrict__ out, int64_t nbytes) {
    const ds_jpeg_desc &d = desc[blockIdx.y];
    dsjpeg::Geometry g;
    if (!usable(d, ncoef, nbytes, scratch_bytes, g)) return;
    dsjpeg::Plane pl[3];
    dsjpeg::planes_of(scratch + d.coef_offset, g, pl);
    const int cw = d.crop_w;
    const int64_t npix = (int64_t)d.crop_h * cw, groups = (npix + 3) >> 2;
    uint8_t *dst = out + d.out_offset;
    for (int64_t gi = (int64_t)blockIdx.x * 256 + threadIdx.x; gi < groups; gi += (int64_t)gridDim.x * 256) {
        const int64_t q0 = gi * 4;
        int y = (int)(q0 / cw), x = (int)(q0 - (int64_t)y * cw);
        const int n = npix - q0 < 4 ? (int)(npix - q0) : 4;
        uint8_t px[12];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            px[3 * k] = px[3 * k + 1] = px[3 * k + 2] = 0;
            if (k < n) dsjpeg::pixel(pl, g, d.y0 + y, d.x0 + x, px + 3 * k);
            if (++x == cw) {
                x = 0;
                ++y;
            }
        }
        if (n == 4) {
            rgb4 w;
            w.a = px[0] | px[1] << 8 | px[2] << 16 | (uint32_t)px[3] << 24;
            w.b = px[4] | px[5] << 8 | px[6] << 16 | (uint32_t)px[7] << 24;
            w.c = px[8] | px[9] << 8 | px[10] << 16 | (uint32_t)px[11] << 24;
            *reinterpret_cast<rgb4 *>(dst + q0 * 3) = w;
        } else {
            for (int k = 0; k < 3 * n; ++k) dst[q0 * 3 + k] = px[k];
        }
    }
}

// ---- ds_jpeg_entropy_decode_device: the Huffman decode of restart-segmented streams ------------------------------------------------
//   jpeg_entropy_kernel   blockIdx.x = image, 256 lanes.  All lanes zero the image's coefficient range with 16-byte stores
//                         while lanes 0..5 build the decoding tables of the (up to) three DC and three AC tables from their
//                         DHT form into LDS (8.3 KB); one barrier; then lane k decodes segments k, k + 256, ... with the
//                         segment decoder of jpeg_common.h, byte by byte from global memory, and stores the non-zero
//                         coefficients through the zig-zag table in LDS.  The eight column sums of the block being decoded
//                         sit in LDS (s_col[c][lane]: consecutive lanes on consecutive banks), the three DC predictors in
//                         named registers.  Lanes diverge freely there: the last barrier is in front of the segment loop.
static_assert(sizeof(ds_jpeg_huff) == 272 && sizeof(ds_jpeg_scan_desc) == 1856 && offsetof(ds_jpeg_scan_desc, quant) == 32 &&
                  offsetof(ds_jpeg_scan_desc, dc) == 224 && offsetof(ds_jpeg_scan_desc, ac) == 1040 && sizeof(ds_jpeg_segment) == 24 &&
                  offsetof(ds_jpeg_segment, first_mcu) == 16,
              "ds_jpeg_scan_desc / ds_jpeg_segment are ABI: ops.jpeg_scan_desc_dtype() / jpeg_segment_dtype() mirror them");

__constant__ uint8_t c_zigzag[64] = DS_JPEG_ZIGZAG_INIT;

constexpr int kEntropyLanes = 256;

__global__ __launch_bounds__(kEntropyLanes) void jpeg_entropy_kernel(const uint8_t *__restrict__ scan, int64_t nscan,
                                                                     const ds_jpeg_scan_desc *__restrict__ images,
                                                                     const ds_jpeg_segment *__restrict__ segs, int64_t nsegs,
                                                                     int16_t *__restrict__ coef, int64_t ncoef,
                                                                     int32_t *__restrict__ status) {
    __shared__ dsjpeg::HuffTable s_tab[6];                 // DC of components 0..2, AC of components 0..2
    __shared__ int32_t s_col[8][kEntropyLanes];
    __shared__ uint8_t s_q[3][64];
    __shared__ uint8_t s_zigzag[64];
    __shared__ int32_t s_err;

    const ds_jpeg_scan_desc &d = images[blockIdx.x];
    const int t = threadIdx.x;
    dsjpeg::Geometry g;
    const bool usable = dsjpeg::scan_desc_ok(d, ncoef, nsegs, g);      // uniform over the workgroup
    if (t == 0) {
        s_err = usable ? 0 : DS_JPEG_E_TABLE;
        status[blockIdx.x] = 0;                            // failing lanes OR their bits in behind the second barrier
    }
    if (t < 64) s_zigzag[t] = c_zigzag[t];
    if (t < 192) s_q[t >> 6][t & 63] = d.quant[t >> 6][t & 63];
    __syncthreads();
    if (usable) {
        uint4 *dst = reinterpret_cast<uint4 *>(coef + d.coef_offset);       // 16-byte aligned: base and offset are
        const int64_t n16 = g.blocks * 8;                                   // 64 int16 = 8 x 16 bytes per block
        for (int64_t i = t; i < n16; i += kEntropyLanes) dst[i] = make_uint4(0, 0, 0, 0);
        if (t < 6 && t % 3 < g.ncomp) {
            const ds_jpeg_huff &h = t < 3 ? d.dc[t] : d.ac[t - 3];
            if (!dsjpeg::huff_build(h.counts, h.values, t < 3, s_tab[t])) atomicOr(&s_err, DS_JPEG_E_TABLE);
        }
    }
    __threadfence();                                       // the zeros are in place before any lane stores a coefficient
    __syncthreads();
    int err = s_err;
    if (usable && !err) {
        dsjpeg::SegmentTables tab;
        tab.dc[0] = &s_tab[0], tab.dc[1] = &s_tab[1], tab.dc[2] = &s_tab[2];
        tab.ac[0] = &s_tab[3], tab.ac[1] = &s_tab[4], tab.ac[2] = &s_tab[5];
        tab.q[0] = s_q[0], tab.q[1] = s_q[1], tab.q[2] = s_q[2];
        tab.zigzag = s_zigzag;
        const int64_t mcus = dsjpeg::mcu_count(g);
        const ds_jpeg_segment *sg = segs + d.first_segment;
        for (int i = t; i < d.segments; i += kEntropyLanes) {
            const ds_jpeg_segment s = sg[i], prev = sg[i ? i - 1 : 0];
            if (!dsjpeg::segment_ok(s, prev, i, d.segments, nscan, mcus)) {
                err |= DS_JPEG_E_TABLE;
                continue;
            }
            err |= dsjpeg::decode_segment(scan + s.begin, scan + s.end, s.first_mcu, s.mcus, g, tab, coef + d.coef_offset,
                                          &s_col[0][t], kEntropyLanes);
        }
    }
    if (err) atomicOr(&status[blockIdx.x], err);
}

}  // namespace

extern "C" int ds_jpeg_reconstruct(const int16_t *coef, int64_t ncoef, const ds_jpeg_desc *desc, int32_t batch,
                                   uint8_t *out_bytes, int64_t nbytes, void *scratch, int64_t scratch_bytes, void *stream) {
    DS_REQUIRE(coef && desc && out_bytes && scratch && ncoef > 0 && nbytes > 0 && batch > 0, "ds_jpeg_reconstruct: bad argument");
    DS_REQUIRE(batch <= 65535, "ds_jpeg_reconstruct: at most 65535 images per launch");
    DS_REQUIRE(((uintptr_t)coef & 15) == 0 && ((uintptr_t)out_bytes & 3) == 0 && ((uintptr_t)scratch & 15) == 0,
               "ds_jpeg_reconstruct: coef and scratch must be 16-byte aligned, out_bytes 4-byte aligned");
    if (scratch_bytes < ncoef) {
        ds::set_error("ds_jpeg_reconstruct: scratch of %lld bytes, %lld needed", (long long)scratch_bytes, (long long)ncoef);
        return DS_ERR_WORKSPACE;
    }
    int gx = ds::kMaxStreamBlocks / batch;
    gx = gx < 1 ? 1 : gx > 64 ? 64 : gx;
    hipLaunchKernelGGL(jpeg_idct_kernel, dim3(gx, batch), dim3(256), 0, (hipStream_t)stream, coef, ncoef, desc, nbytes,
                       (uint8_t *)scratch, scratch_bytes);
    hipLaunchKernelGGL(jpeg_colour_kernel, dim3(gx, batch), dim3(256), 0, (hipStream_t)stream, (const uint8_t *)scratch,
                       scratch_bytes, desc, ncoef, out_bytes, nbytes);
    return ds::check_launch("ds_jpeg_reconstruct");
}

extern "C" int ds_jpeg_entropy_decode_device(const uint8_t *scan, int64_t nscan, const ds_jpeg_scan_desc *images, int32_t nimages,
                                             const ds_jpeg_segment *segs, int64_t nsegs, int16_t *coef, int64_t ncoef,
                                             int32_t *status, void *stream) {
    DS_REQUIRE(scan && images && segs && coef && status && nscan > 0 && nsegs > 0 && ncoef > 0 && nimages > 0,
               "ds_jpeg_entropy_decode_device: bad argument");
    DS_REQUIRE(nimages <= 65535, "ds_jpeg_entropy_decode_device: at most 65535 images per launch");
    DS_REQUIRE(((uintptr_t)coef & 15) == 0 && ((uintptr_t)images & 7) == 0 && ((uintptr_t)segs & 7) == 0 && ((uintptr_t)status & 3) == 0,
               "ds_jpeg_entropy_decode_device: coef must be 16-byte aligned, the tables 8-byte, status 4-byte");
    hipLaunchKernelGGL(jpeg_entropy_kernel, dim3(nimages), dim3(kEntropyLanes), 0, (hipStream_t)stream, scan, nscan, images, segs,
                       nsegs, coef, ncoef, status);
    return ds::check_launch("ds_jpeg_entropy_decode_device");
}
