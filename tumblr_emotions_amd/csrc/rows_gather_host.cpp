// ds_rows_gather_host: the CPU statement of ds_rows_gather (rows_gather.hip), plain C++ on host pointers of any
// alignment.  The argument test, the test of an index and the place a unit comes from are rows_gather_common.h's, shared
// with the kernel; what is left here is one loop that stores each 4-byte unit of each usable row once, bytewise.
#include <stdint.h>

#include "ds_kernels.h"
#include "rows_gather_common.h"

namespace ds {
void set_error(const char *fmt, ...);
}

extern "C" int ds_rows_gather_host(const ds_rows_table *tables, int32_t ntables, const int64_t *index, int64_t n, int64_t nrows) {
    if (const char *bad = dsrows::args_error(tables, ntables, index, n, nrows)) {
        ds::set_error("ds_rows_gather_host: %s", bad);
        return DS_ERR_ARG;
    }
    const uint8_t *ix = reinterpret_cast<const uint8_t *>(index);
    for (int32_t t = 0; t < ntables; ++t) {
        const uint8_t *src = static_cast<const uint8_t *>(tables[t].src);
        uint8_t *dst = static_cast<uint8_t *>(tables[t].dst);
        const int64_t row_bytes = tables[t].row_bytes;
        const uint32_t row_units = (uint32_t)(row_bytes / 4), units = (uint32_t)(n * row_units);
        for (uint32_t u = 0; u < units; ++u) {
            uint32_t i, k;
            dsrows::split_unit(u, row_units, i, k);
            int64_t row = 0;
            for (int b = 7; b >= 0; --b) row = (int64_t)(((uint64_t)row << 8) | ix[(int64_t)i * 8 + b]);      // little endian, any alignment
            if (!dsrows::row_ok(row, nrows)) continue;
            const uint8_t *s = src + dsrows::unit_offset(row, row_bytes, k, 4);
            uint8_t *d = dst + dsrows::unit_offset(i, row_bytes, k, 4);
            for (int b = 0; b < 4; ++b) d[b] = s[b];
        }
    }
    return DS_OK;
}
