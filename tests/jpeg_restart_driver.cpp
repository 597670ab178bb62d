// Stand-alone driver of the restart-segment entry points of tumblr_emotions_amd/csrc/jpeg_host.cpp for
// tests/test_jpeg_restart_sanitized_cpu.py: built with the host compiler and -fsanitize=address,undefined, linked with
// jpeg_host.cpp only.  Every file of the list goes through ds_jpeg_scan, ds_jpeg_restart_transcode and
// ds_jpeg_entropy_decode_segments_host intact (all three must succeed, the segment decoder must give the coefficients of
// ds_jpeg_entropy_decode, and so must the transcoded stream: exit 2 otherwise), as `mutations` copies with one seeded
// single-byte change inside the scan each, and at every truncation of up to `max_cut` bytes.  Damaged input may decode, be
// unsupported or be flagged -- it must never crash or trip a sanitizer.  Every buffer is an exact-size heap allocation, so a
// read or a store past its end is a report.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "ds_kernels.h"

static uint64_t g_state;
static uint32_t next_u32() {              // a 64-bit LCG (Knuth's MMIX constants), high half
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(g_state >> 32);
}

static long g_ok = 0, g_rejected = 0, g_flagged = 0, g_transcoded = 0;

struct Scanned {
    int rc;
    ds_jpeg_info info;
    ds_jpeg_scan_info scan;
    std::vector<int64_t> cuts;
};

static Scanned scan_of(const uint8_t *bytes, size_t n) {
    Scanned s;
    int64_t one[1];
    s.rc = ds_jpeg_scan(bytes, (int64_t)n, &s.info, &s.scan, one, 1);
    if (s.rc == DS_JPEG_MORE || s.rc == DS_OK) {
        s.cuts.resize((size_t)s.scan.cut_count);
        s.rc = ds_jpeg_scan(bytes, (int64_t)n, &s.info, &s.scan, s.cuts.data(), (int64_t)s.cuts.size());
    }
    return s;
}

// the segments of a scanned stream through ds_jpeg_entropy_decode_segments_host, tables as the loader builds them;
// returns the status word, -1 when the stream does not scan; `coef_out` receives the coefficients
static int decode_segments(const uint8_t *bytes, size_t n, std::vector<int16_t> *coef_out) {
    const Scanned s = scan_of(bytes, n);
    if (s.rc != DS_OK) return -1;
    const int64_t begin = s.scan.scan_begin, end = s.cuts.back();
    const size_t nscan = (size_t)(end - begin);
    uint8_t *scan = (uint8_t *)malloc(nscan ? nscan : 1);
    memcpy(scan, bytes + begin, nscan);
    ds_jpeg_scan_desc *d = (ds_jpeg_scan_desc *)calloc(1, sizeof(ds_jpeg_scan_desc));
    d->width = s.info.width, d->height = s.info.height, d->sampling = s.info.sampling;
    d->segments = (int32_t)s.cuts.size();
    memcpy(d->quant, s.info.quant, sizeof(d->quant));
    memcpy(d->dc, s.scan.dc, sizeof(d->dc));
    memcpy(d->ac, s.scan.ac, sizeof(d->ac));
    const int hs = s.info.sampling == DS_JPEG_422 || s.info.sampling == DS_JPEG_420 ? 2 : 1, vs = s.info.sampling == DS_JPEG_420 ? 2 : 1;
    const int64_t mcus = (int64_t)((s.info.width + 8 * hs - 1) / (8 * hs)) * ((s.info.height + 8 * vs - 1) / (8 * vs));
    const int64_t interval = s.info.restart_interval ? s.info.restart_interval : mcus;
    ds_jpeg_segment *segs = (ds_jpeg_segment *)calloc(s.cuts.size(), sizeof(ds_jpeg_segment));
    for (size_t i = 0; i < s.cuts.size(); ++i) {
        segs[i].begin = i ? s.cuts[i - 1] + 2 - begin : 0;
        segs[i].end = s.cuts[i] - begin;
        segs[i].first_mcu = (int32_t)(i * interval);
        segs[i].mcus = (int32_t)(mcus - (int64_t)i * interval < interval ? mcus - (int64_t)i * interval : interval);
    }
    int16_t *coef = (int16_t *)malloc((size_t)s.info.coef_bytes);
    int32_t status = -1;
    const int rc = ds_jpeg_entropy_decode_segments_host(scan, (int64_t)nscan, d, 1, segs, (int64_t)s.cuts.size(), coef,
                                                        s.info.coef_count, &status);
    if (rc != DS_OK) status = -2;
    if (coef_out) coef_out->assign(coef, coef + s.info.coef_count);
    free(coef);
    free(segs);
    free(d);
    free(scan);
    return status;
}

// all three entry points on one (possibly damaged) stream; `intact`: everything must succeed and agree
static int run(const uint8_t *src, size_t n, bool intact) {
    uint8_t *bytes = (uint8_t *)malloc(n ? n : 1);           // exact size: the sanitizer sees any overrun
    memcpy(bytes, src, n);
    std::vector<int16_t> got;
    const int status = decode_segments(bytes, n, &got);
    if (status == 0) ++g_ok; else if (status < 0) ++g_rejected; else ++g_flagged;
    // the stream decoder's verdict is the segment decoder's
    ds_jpeg_info info;
    std::vector<int16_t> want;
    int host = DS_JPEG_UNSUPPORTED;
    if (ds_jpeg_probe(bytes, (int64_t)n, &info) == DS_OK) {
        want.resize((size_t)info.coef_count);
        host = ds_jpeg_entropy_decode(bytes, (int64_t)n, &info, want.data(), info.coef_count);
    }
    int bad = 0;
    if ((status == 0) != (host == DS_OK) || (status == 0 && got != want)) bad = 3;
    if (status == -2) bad = 4;
    // the transcoder: first with no room (it must ask for it), then with exactly what it asked for
    for (int interval = 0; interval <= 3 && !bad; interval += 3) {
        int64_t need = 0;
        int rc = ds_jpeg_restart_transcode(bytes, (int64_t)n, interval, nullptr, 0, &need);
        if ((rc == DS_JPEG_MORE) != (host == DS_OK)) bad = 5;
        if (rc != DS_JPEG_MORE) continue;
        uint8_t *out = (uint8_t *)malloc((size_t)need);
        rc = ds_jpeg_restart_transcode(bytes, (int64_t)n, interval, out, need, &need);
        std::vector<int16_t> again;
        if (rc != DS_OK || decode_segments(out, (size_t)need, &again) != 0 || again != want) bad = 6;
        ++g_transcoded;
        free(out);
    }
    free(bytes);
    if (intact && (status != 0 || host != DS_OK)) bad = 2;
    return bad;
}

int main(int argc, char **argv) {
    if (argc != 5) {
        fprintf(stderr, "usage: %s <list file> <mutations> <max cut> <seed>\n", argv[0]);
        return 64;
    }
    const int mutations = atoi(argv[2]), max_cut = atoi(argv[3]);
    g_state = strtoull(argv[4], nullptr, 10);
    FILE *list = fopen(argv[1], "r");
    if (!list) return 65;
    char path[4096];
    long files = 0;
    while (fgets(path, sizeof(path), list)) {
        path[strcspn(path, "\r\n")] = 0;
        if (!path[0]) continue;
        FILE *f = fopen(path, "rb");
        if (!f) return 66;
        std::vector<uint8_t> data;
        uint8_t chunk[65536];
        size_t got;
        while ((got = fread(chunk, 1, sizeof(chunk), f)) > 0) data.insert(data.end(), chunk, chunk + got);
        fclose(f);
        ++files;
        int bad = run(data.data(), data.size(), true);
        if (bad) {
            fprintf(stderr, "%s: the intact file failed (%d)\n", path, bad);
            return bad;
        }
        const Scanned s = scan_of(data.data(), data.size());
        const size_t lo = (size_t)s.scan.scan_begin, hi = (size_t)s.cuts.back();
        std::vector<uint8_t> m(data);
        for (int k = 0; k < mutations && hi > lo; ++k) {
            const size_t at = lo + next_u32() % (hi - lo);
            const uint8_t keep = m[at];
            m[at] = (uint8_t)(keep ^ (1 + next_u32() % 255));
            if ((bad = run(m.data(), m.size(), false))) {
                fprintf(stderr, "%s: mutation %d at %zu: the decoders disagree (%d)\n", path, k, at, bad);
                return bad;
            }
            m[at] = keep;
        }
        for (size_t cut = 0; cut <= (size_t)max_cut && cut < data.size(); ++cut)
            if ((bad = run(data.data(), cut, false))) {
                fprintf(stderr, "%s: cut %zu: the decoders disagree (%d)\n", path, cut, bad);
                return bad;
            }
    }
    fclose(list);
    printf("files %ld decoded %ld flagged %ld rejected %ld transcoded %ld\n", files, g_ok, g_flagged, g_rejected, g_transcoded);
    return 0;
}
