// ds_rows_gather: the batch assembly of the Mixed_5b feature cache.  ONE launch copies, for up to 8 resident tables that
// share a row count, the rows index[0 .. n) into the batch buffers: dst_t[i] = src_t[index[i]].  The tables travel by
// value in the kernel arguments; the index vector stays on the device (a slice of the epoch's permutation).
//
//   rows_gather_kernel  a one-dimensional grid, cut into one run of workgroups per table: the feature table (163 072 B a
//                       row) gets up to ds::kMaxStreamBlocks workgroups, the 400-byte and 8-byte tables one or a few.  A
//                       run walks its table as a flat [n, row_units] array of 16-byte units (4-byte units when the row
//                       length or a base address is not a multiple of 16): consecutive lanes own consecutive units, a
//                       lane moves kPerLane units per turn -- all loads issued before the first store -- and the run
//                       grid-strides.  Source units are read once per pass over the data set (non-temporal loads); the
//                       destination is what the next kernel reads (plain stores).  Exactly one lane stores each
//                       destination unit of a row whose index is inside [0, nrows); a row whose index is not gets no
//                       store in any table.  No atomics, no LDS.  The address arithmetic is rows_gather_common.h's,
//                       shared with the host statement (rows_gather_host.cpp).
#include "ds_common.h"
#include "rows_gather_common.h"

namespace {

constexpr uint32_t kPerLane = 4, kTurn = 256u * kPerLane;        // units per lane and per workgroup in one turn

struct RowsRun {
    const uint8_t *src;
    uint8_t *dst;
    int64_t row_bytes;
    uint32_t row_units, units;        // units per row; n * row_units
    uint32_t unit;                    // 16 or 4
    uint32_t first_block, blocks;     // the run's workgroups: [first_block, first_block + blocks)
};

struct RowsArgs {
    RowsRun run[dsrows::kMaxTables];
    int32_t ntables;
};

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

template <typename V>
__device__ __forceinline__ void rows_walk(const RowsRun &r, const int64_t *__restrict__ index, int64_t nrows, uint32_t block) {
    for (uint32_t base = block * kTurn; base < r.units; base += r.blocks * kTurn) {      // units <= 2^31: no wrap
        V v[kPerLane];
        int64_t to[kPerLane];
#pragma unroll
        for (uint32_t j = 0; j < kPerLane; ++j) {
            const uint32_t u = base + j * 256u + threadIdx.x;
            to[j] = -1;
            if (u < r.units) {
                uint32_t i, k;
                dsrows::split_unit(u, r.row_units, i, k);
                const int64_t row = index[i];
                if (dsrows::row_ok(row, nrows)) {
                    v[j] = __builtin_nontemporal_load(reinterpret_cast<const V *>(r.src + dsrows::unit_offset(row, r.row_bytes, k, sizeof(V))));
                    to[j] = dsrows::unit_offset(i, r.row_bytes, k, sizeof(V));
                }
            }
        }
#pragma unroll
        for (uint32_t j = 0; j < kPerLane; ++j)
            if (to[j] >= 0) *reinterpret_cast<V *>(r.dst + to[j]) = v[j];
    }
}

__global__ __launch_bounds__(256) void rows_gather_kernel(RowsArgs a, const int64_t *__restrict__ index, int64_t nrows) {
    RowsRun r = a.run[0];                 // the run this workgroup belongs to: uniform selects, no indexed kernel argument
#pragma unroll
    for (int t = 1; t < dsrows::kMaxTables; ++t)
        if (t < a.ntables && blockIdx.x >= a.run[t].first_block) r = a.run[t];
    const uint32_t block = blockIdx.x - r.first_block;
    if (r.unit == 16u)
        rows_walk<u32x4>(r, index, nrows, block);
    else
        rows_walk<uint32_t>(r, index, nrows, block);
}

}  // namespace

extern "C" int ds_rows_gather(const ds_rows_table *tables, int32_t ntables, const int64_t *index, int64_t n, int64_t nrows,
                              void *stream) {
    const char *bad = dsrows::args_error(tables, ntables, index, n, nrows);
    DS_REQUIRE(!bad, "ds_rows_gather: %s", bad);
    DS_REQUIRE(((uintptr_t)index & 7) == 0, "ds_rows_gather: index must be 8-byte aligned");
    RowsArgs a = {};
    a.ntables = ntables;
    uint32_t grid = 0;
    for (int32_t t = 0; t < ntables; ++t) {
        DS_REQUIRE((((uintptr_t)tables[t].src | (uintptr_t)tables[t].dst) & 3) == 0, "ds_rows_gather: src and dst must be 4-byte aligned");
        RowsRun &r = a.run[t];
        r.src = static_cast<const uint8_t *>(tables[t].src);
        r.dst = static_cast<uint8_t *>(tables[t].dst);
        r.row_bytes = tables[t].row_bytes;
        r.unit = dsrows::unit_bytes(tables[t]);
        r.row_units = (uint32_t)(r.row_bytes / r.unit);
        r.units = (uint32_t)(n * r.row_units);
        r.first_block = grid;
        r.blocks = (uint32_t)ds::stream_grid(r.units, kTurn);
        grid += r.blocks;
    }
    hipLaunchKernelGGL(rows_gather_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, a, index, nrows);
    return ds::check_launch("ds_rows_gather");
}
