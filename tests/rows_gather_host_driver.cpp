// Stand-alone driver of ds_rows_gather_host for the sanitised build (tests/test_feature_cache_cpu.py): its own main, linked
// with csrc/rows_gather_host.cpp alone.  Random launches -- 1..8 tables, row lengths of 4 .. 163 072 bytes, repeated and
// out-of-range indices, every pointer (the index vector too) at an odd byte offset inside an exactly sized heap block, so
// that a byte read or written outside a table, a destination or the index vector is the sanitizer's to report -- each
// checked against a plain loop.  argv: launches seed.  Prints "launches N rows_copied C rows_skipped S".
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <random>
#include <vector>

#include "ds_kernels.h"

namespace ds {
static char g_err[256];
void set_error(const char *fmt, ...) { strncpy(g_err, fmt, sizeof(g_err) - 1); }      // (what error.cpp does in the library)
}  // namespace ds

int main(int argc, char **argv) {
    const int launches = argc > 1 ? atoi(argv[1]) : 100;
    std::mt19937_64 rng(argc > 2 ? strtoull(argv[2], nullptr, 10) : 1);
    const int64_t lengths[] = {4, 8, 20, 400, 163072, 12, 1024, 36};
    long copied = 0, skipped = 0;
    for (int l = 0; l < launches; ++l) {
        const int ntables = 1 + (int)(rng() % 8);
        const int64_t nrows = 1 + (int64_t)(rng() % 9), n = 1 + (int64_t)(rng() % 7);
        std::vector<int64_t> index(n);
        for (auto &r : index) {
            const uint64_t k = rng() % 10;
            r = k == 0 ? -1 - (int64_t)(rng() % 5) : k == 1 ? nrows + (int64_t)(rng() % 5) : k == 2 ? INT64_MAX : (int64_t)(rng() % nrows);
        }
        const size_t ioff = 1 + rng() % 7;
        std::vector<uint8_t *> blocks;
        uint8_t *iblock = (uint8_t *)malloc(ioff + 8 * n);              // exactly sized: the last index ends the block
        blocks.push_back(iblock);
        memcpy(iblock + ioff, index.data(), 8 * n);
        ds_rows_table tables[8];
        std::vector<std::vector<uint8_t>> want;
        for (int t = 0; t < ntables; ++t) {
            const int64_t rb = lengths[rng() % 8];
            const size_t soff = 1 + rng() % 15, doff = 1 + rng() % 15;
            uint8_t *s = (uint8_t *)malloc(soff + nrows * rb), *d = (uint8_t *)malloc(doff + n * rb);
            blocks.push_back(s);
            blocks.push_back(d);
            for (int64_t b = 0; b < nrows * rb; ++b) s[soff + b] = (uint8_t)rng();
            memset(d + doff, 0xA5, n * rb);
            tables[t] = {s + soff, d + doff, rb};
            std::vector<uint8_t> w(n * rb, 0xA5);
            for (int64_t i = 0; i < n; ++i)
                if (index[i] >= 0 && index[i] < nrows) memcpy(w.data() + i * rb, s + soff + index[i] * rb, rb);
            want.push_back(w);
        }
        const int rc = ds_rows_gather_host(tables, ntables, (const int64_t *)(iblock + ioff), n, nrows);
        if (rc != DS_OK) {
            fprintf(stderr, "launch %d: rc %d\n", l, rc);
            return 2;
        }
        for (int t = 0; t < ntables; ++t)
            if (memcmp(tables[t].dst, want[t].data(), want[t].size())) {
                fprintf(stderr, "launch %d table %d (row_bytes %lld) differs\n", l, t, (long long)tables[t].row_bytes);
                return 3;
            }
        for (int64_t i = 0; i < n; ++i) (index[i] >= 0 && index[i] < nrows ? copied : skipped) += 1;
        for (uint8_t *b : blocks) free(b);
    }
    ds_rows_table bad = {nullptr, nullptr, 8};
    const int64_t zero = 0;
    if (ds_rows_gather_host(&bad, 1, &zero, 1, 1) != DS_ERR_ARG || ds_rows_gather_host(nullptr, 1, &zero, 1, 1) != DS_ERR_ARG) return 4;
    printf("launches %d rows_copied %ld rows_skipped %ld\n", launches, copied, skipped);
    return 0;
}
