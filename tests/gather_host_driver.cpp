// Stand-alone driver of ds_ragged_gather_host for the sanitised build (tests/test_input_cache_cpu.py): its own main, linked
// with csrc/gather_host.cpp only.  Every buffer is a heap allocation of EXACTLY the size the call is told, so that a byte
// read or written outside it is an AddressSanitizer report.
//   usage: gather_host_driver <random descriptors> <seed>
// (1) the grid of the Python test: six source sizes, whole-image / corner / x0 = 1, 2, 3 / width 1..9 windows, source
//     offsets 0, 16, 80, source buffers that end at the last byte a window reads; batches of one and of seven over both
//     sources.  The output must equal plain indexing, the guard bytes and the gaps must keep their pattern.
// (2) random descriptors, most of them out of range somewhere: a record either is copied exactly or leaves `out` untouched.
// Prints "grid <launches> copied <n> skipped <n>"; exit status 1 on any mismatch.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "ds_kernels.h"

namespace {

uint64_t g_state = 1;
uint32_t rnd() {                                 // xorshift64*
    g_state ^= g_state >> 12;
    g_state ^= g_state << 25;
    g_state ^= g_state >> 27;
    return (uint32_t)((g_state * 2685821237242563821ull) >> 32);
}
int rnd_in(int lo, int hi) { return (int)((int64_t)lo + rnd() % (uint32_t)((int64_t)hi - lo + 1)); }

uint8_t pattern(int64_t i) { return (uint8_t)((i * 7 + 3) % 251); }

struct Window {
    int y0, x0, h, w;
};

// an independent statement of the contract for one record: false = it must be skipped
bool fits(const ds_gather_desc &d, int64_t narena, int64_t nspill, int64_t nout) {
    if (d.src != 0 && d.src != 1) return false;
    if (d.height < 1 || d.width < 1 || d.y0 < 0 || d.x0 < 0 || d.pitch < 1) return false;
    const int64_t n = (int64_t)d.height * d.width * 3, nsrc = d.src ? nspill : narena;
    if (n > 0x7fffffff || ((int64_t)d.x0 + d.width) * 3 > d.pitch) return false;
    if (d.src_offset < 0 || d.src_offset > nsrc) return false;                  // (compared without forming sums that could overflow)
    if (((int64_t)d.y0 + d.height - 1) * d.pitch + ((int64_t)d.x0 + d.width) * 3 > nsrc - d.src_offset) return false;
    return d.out_offset >= 0 && d.out_offset % 4 == 0 && d.out_offset <= nout && n <= nout - d.out_offset;
}

int g_fail = 0;

// run one launch on exact-size heap copies and compare with plain indexing; returns the number of records copied
int launch(const std::vector<uint8_t> &arena, const std::vector<uint8_t> &spill, bool have_spill, const std::vector<ds_gather_desc> &desc,
           int64_t nout) {
    const int64_t guard = 64;
    uint8_t *a = (uint8_t *)malloc(arena.size() ? arena.size() : 1), *s = have_spill ? (uint8_t *)malloc(spill.size() ? spill.size() : 1) : nullptr;
    uint8_t *big = (uint8_t *)malloc(guard + nout + guard);
    ds_gather_desc *dd = (ds_gather_desc *)malloc(desc.size() * sizeof(ds_gather_desc));
    if (arena.size()) memcpy(a, arena.data(), arena.size());
    if (s && spill.size()) memcpy(s, spill.data(), spill.size());
    memcpy(dd, desc.data(), desc.size() * sizeof(ds_gather_desc));
    std::vector<uint8_t> want(guard + nout + guard);
    for (int64_t i = 0; i < (int64_t)want.size(); ++i) big[i] = want[i] = pattern(i);
    int copied = 0;
    const int64_t nspill = have_spill ? (int64_t)spill.size() : 0;
    for (const ds_gather_desc &d : desc) {
        if (!fits(d, (int64_t)arena.size(), nspill, nout)) continue;
        ++copied;
        const std::vector<uint8_t> &src = d.src ? spill : arena;
        for (int y = 0; y < d.height; ++y)
            for (int x = 0; x < d.width; ++x)
                for (int c = 0; c < 3; ++c)
                    want[guard + d.out_offset + ((int64_t)y * d.width + x) * 3 + c] =
                        src[d.src_offset + (int64_t)(d.y0 + y) * d.pitch + (int64_t)(d.x0 + x) * 3 + c];
    }
    // out points INTO the guarded block so that a store outside [0, nout) lands on pattern bytes and is seen below;
    // a store outside the whole block is the sanitizer's to report
    const int rc = ds_ragged_gather_host(a, (int64_t)arena.size(), s, nspill, dd, (int32_t)desc.size(), big + guard, nout);
    if (rc != DS_OK || memcmp(big, want.data(), want.size()) != 0) {
        fprintf(stderr, "mismatch: rc %d, %zu records, nout %lld\n", rc, desc.size(), (long long)nout);
        g_fail = 1;
    }
    free(a);
    free(s);
    free(big);
    free(dd);
    return copied;
}

std::vector<Window> windows(int h, int w) {
    std::vector<Window> out = {{0, 0, h, w}, {0, 0, 1, 1}, {0, w - 1, 1, 1}, {h - 1, 0, 1, 1}, {h - 1, w - 1, 1, 1}};
    for (int x0 = 1; x0 <= 3; ++x0)
        if (x0 < w) {
            out.push_back({0, x0, h, w - x0});
            out.push_back({h / 2, x0, h - h / 2, 1});
        }
    for (int ww = 1; ww <= 9; ++ww)
        if (ww <= w) {
            const int y0 = h > 1 ? 1 : 0, x0 = w - ww < 2 ? w - ww : 2;
            out.push_back({y0, x0, h - y0, ww});
        }
    return out;
}

std::vector<uint8_t> noise(int64_t n) {
    std::vector<uint8_t> v((size_t)n);
    for (auto &b : v) b = (uint8_t)rnd();
    return v;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: %s <random descriptors> <seed>\n", argv[0]);
        return 2;
    }
    const int randoms = atoi(argv[1]);
    g_state = strtoull(argv[2], nullptr, 10) | 1;
    const int sizes[6][2] = {{1, 1}, {1, 7}, {7, 1}, {3, 5}, {17, 9}, {64, 48}};
    const int64_t offsets[3] = {0, 16, 80};
    int grid = 0;
    for (auto &hw : sizes)
        for (const Window &win : windows(hw[0], hw[1]))
            for (int64_t off : offsets)
                for (int src = 0; src < 2; ++src) {
                    const int pitch = 3 * hw[1];
                    const int64_t need = off + (int64_t)(win.y0 + win.h - 1) * pitch + (int64_t)(win.x0 + win.w) * 3;
                    const ds_gather_desc d = {off, 0, src, pitch, win.y0, win.x0, win.h, win.w};
                    const int64_t nout = ((int64_t)win.h * win.w * 3 + 3) / 4 * 4;
                    if (launch(src ? noise(16) : noise(need), src ? noise(need) : noise(0), src == 1, {d}, nout) != 1) g_fail = 1;
                    ++grid;
                }
    for (int b = 0; b < 40; ++b) {                // batches of seven over both sources
        std::vector<ds_gather_desc> desc;
        int64_t at[2] = {0, 0}, need[2] = {0, 0}, pos = 0;
        for (int i = 0; i < 7; ++i) {
            const int k = rnd_in(0, 5), src = i ? rnd_in(0, 1) : b & 1, pitch = 3 * sizes[k][1];
            const std::vector<Window> wins = windows(sizes[k][0], sizes[k][1]);
            const Window win = wins[rnd() % wins.size()];
            if (i == 2) pos += 8;
            desc.push_back({at[src], pos, src, pitch, win.y0, win.x0, win.h, win.w});
            const int64_t end = at[src] + (int64_t)(win.y0 + win.h - 1) * pitch + (int64_t)(win.x0 + win.w) * 3;
            need[src] = end > need[src] ? end : need[src];
            at[src] += ((int64_t)sizes[k][0] * pitch + 15) / 16 * 16 + 16 * rnd_in(0, 2);
            pos = (pos + (int64_t)win.h * win.w * 3 + 3) / 4 * 4;
        }
        if (launch(noise(need[0] ? need[0] : 16), noise(need[1]), need[1] > 0, desc, pos) != 7) g_fail = 1;
        ++grid;
    }
    // random records against small buffers: offsets, origins and sizes around every bound, negative and huge values too
    int copied = 0, skipped = 0;
    for (int r = 0; r < randoms; ++r) {
        const int64_t narena = rnd_in(0, 4000), nspill = rnd_in(0, 2000), nout = rnd_in(0, 3000);
        const bool have_spill = rnd() % 4 != 0;
        ds_gather_desc d;
        d.width = rnd() % 16 == 0 ? rnd_in(-2, 0x7fffffff) : rnd_in(0, 24);
        d.height = rnd() % 16 == 0 ? rnd_in(-2, 0x7fffffff) : rnd_in(0, 30);
        d.x0 = rnd() % 16 == 0 ? rnd_in(-3, 0x7fffffff) : rnd_in(0, 6);
        d.y0 = rnd() % 16 == 0 ? rnd_in(-3, 0x7fffffff) : rnd_in(0, 6);
        d.pitch = rnd() % 8 == 0 ? rnd_in(-1, 0x7fffffff) : (int32_t)(3 * ((int64_t)d.width + d.x0 + rnd_in(-1, 3)) & 0x7fffffff);
        d.src = rnd() % 10 == 0 ? rnd_in(-1, 3) : rnd_in(0, 1);
        d.src_offset = rnd() % 10 == 0 ? (int64_t)(rnd() >> 2) * (rnd() >> 2) - (1ll << 40) : rnd_in(-4, 1200);
        d.out_offset = rnd() % 10 == 0 ? (int64_t)(rnd() >> 2) * (rnd() >> 2) - (1ll << 40) : rnd_in(-1, 300) * (rnd() % 8 ? 4 : 1);
        const int got = launch(noise(narena), noise(nspill), have_spill, {d}, nout);
        copied += got;
        skipped += 1 - got;
    }
    printf("grid %d copied %d skipped %d\n", grid, copied, skipped);
    return g_fail;
}
