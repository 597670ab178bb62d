// The address arithmetic of ds_ragged_gather, ONE definition for the host statement (ds_ragged_gather_host, plain C++)
// and the kernel (gather_bytes.hip): which descriptors are usable, and where destination byte k of a window comes from.
#pragma once
#include <stdint.h>
#include "ds_kernels.h"

#if defined(__HIPCC__)
#define DS_GATHER_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define DS_GATHER_HD inline
#endif

namespace dsgather {

// bytes of the window; 0 when the record's own numbers are unusable (a window is < 2^31 bytes: 32-bit row arithmetic)
DS_GATHER_HD int64_t window_bytes(const ds_gather_desc &d) {
    if (d.height < 1 || d.width < 1 || d.y0 < 0 || d.x0 < 0 || d.pitch < 1) return 0;
    const int64_t n = (int64_t)d.height * d.width * 3;
    return n > 0x7fffffff ? 0 : n;
}

// the record is usable: a known source that exists, every source byte of the window inside that source's n bytes, the
// window's rows inside the pitch, every destination byte inside nout, an aligned start -- all in 64 bits
DS_GATHER_HD bool desc_ok(const ds_gather_desc &d, int64_t narena, int64_t nspill, int64_t nout) {
    const int64_t n = window_bytes(d);
    if (!n || (d.src != 0 && d.src != 1)) return false;
    const int64_t nsrc = d.src ? nspill : narena;
    if (((int64_t)d.x0 + d.width) * 3 > d.pitch || d.src_offset < 0 || d.src_offset > nsrc) return false;
    const int64_t last = ((int64_t)d.y0 + d.height - 1) * d.pitch + ((int64_t)d.x0 + d.width) * 3;      // one past the last byte read
    if (last > nsrc - d.src_offset) return false;
    return d.out_offset >= 0 && !(d.out_offset & 3) && d.out_offset <= nout && n <= nout - d.out_offset;
}

// first source byte of the window: pixel (y0, x0)
DS_GATHER_HD int64_t window_origin(const ds_gather_desc &d) { return d.src_offset + (int64_t)d.y0 * d.pitch + (int64_t)d.x0 * 3; }

// the source byte (from the window's origin) of byte b of window row y
DS_GATHER_HD int64_t row_byte(const ds_gather_desc &d, uint32_t y, uint32_t b) { return (int64_t)y * d.pitch + b; }

// the source byte (from the window's origin) that destination byte k of the flat window holds
DS_GATHER_HD int64_t source_byte(const ds_gather_desc &d, uint32_t k) {
    const uint32_t rowbytes = (uint32_t)d.width * 3u, y = k / rowbytes;
    return row_byte(d, y, k - y * rowbytes);
}

}  // namespace dsgather
