// The address arithmetic of ds_rows_gather, ONE definition for the host statement (ds_rows_gather_host, plain C++) and
// the kernel (rows_gather.hip): which launches are usable, which index names a row, and where unit k of destination
// row i comes from.  A table is walked in units of 16 or 4 bytes; unit u of the flat [n, row_units] walk is unit
// u % row_units of destination row u / row_units.
#pragma once
#include <stdint.h>
#include "ds_kernels.h"

#if defined(__HIPCC__)
#define DS_ROWS_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define DS_ROWS_HD inline
#endif

namespace dsrows {

constexpr int kMaxTables = 8;
constexpr int64_t kMaxUnits = (int64_t)1 << 31;        // units of one table in one launch: the flat walk is 32-bit

// the arguments are usable (nothing is read through a pointer here); text of the first complaint otherwise
DS_ROWS_HD const char *args_error(const ds_rows_table *tables, int32_t ntables, const int64_t *index, int64_t n, int64_t nrows) {
    if (!tables || ntables < 1 || ntables > kMaxTables) return "1 to 8 tables";
    if (!index || n < 1 || nrows < 1) return "an index vector, n >= 1 and nrows >= 1";
    for (int32_t t = 0; t < ntables; ++t) {
        if (!tables[t].src || !tables[t].dst) return "a null table";
        if (tables[t].row_bytes < 4 || (tables[t].row_bytes & 3)) return "row_bytes must be a positive multiple of 4";
        if (tables[t].row_bytes / 4 > kMaxUnits / n) return "more than 2^31 units of one table in one launch";
    }
    return nullptr;
}

// bytes per unit of a table: 16 when the row length and both base addresses allow it, 4 otherwise
DS_ROWS_HD uint32_t unit_bytes(const ds_rows_table &t) {
    return !(t.row_bytes & 15) && !(((uintptr_t)t.src | (uintptr_t)t.dst) & 15) ? 16u : 4u;
}

// index value `row` names a row of the tables
DS_ROWS_HD bool row_ok(int64_t row, int64_t nrows) { return (uint64_t)row < (uint64_t)nrows; }

// flat unit u -> destination row i and unit k of that row
DS_ROWS_HD void split_unit(uint32_t u, uint32_t row_units, uint32_t &i, uint32_t &k) {
    i = u / row_units;
    k = u - i * row_units;
}

// byte offset of unit k of row r, 64-bit (a feature table is far beyond 4 GiB)
DS_ROWS_HD int64_t unit_offset(int64_t r, int64_t row_bytes, uint32_t k, uint32_t unit) { return r * row_bytes + (int64_t)k * unit; }

}  // namespace dsrows
