// Stand-alone driver of tumblr_emotions_amd/csrc/jpeg_host.cpp for tests/test_jpeg_host_sanitized_cpu.py: built with the host
// compiler and -fsanitize=address,undefined, linked with jpeg_host.cpp only.  For every file of the list it decodes the file
// itself (which must succeed: exit 2 otherwise), `mutations` copies with one seeded single-byte change each and every
// truncation of up to `max_cut` bytes.  Damaged input may decode, be unsupported or be an argument error -- it must never
// crash or trip a sanitizer.  Each buffer is an exact-size heap allocation, so a read past `n` is a report.
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

static long g_ok = 0, g_unsupported = 0;

// probe + entropy decode + host reconstruction of the whole image; returns 0 when pixels came out
static int decode(const uint8_t *src, size_t n) {
    uint8_t *bytes = (uint8_t *)malloc(n ? n : 1);           // exact size: the sanitizer sees any overrun
    memcpy(bytes, src, n);
    ds_jpeg_info info;
    int rc = ds_jpeg_probe(bytes, (int64_t)n, &info);
    if (rc == DS_OK) {
        int16_t *coef = (int16_t *)malloc((size_t)info.coef_bytes);
        rc = ds_jpeg_entropy_decode(bytes, (int64_t)n, &info, coef, info.coef_count);
        if (rc == DS_OK) {
            ds_jpeg_desc d;
            memset(&d, 0, sizeof(d));
            d.width = info.width, d.height = info.height, d.sampling = info.sampling;
            d.crop_h = info.height, d.crop_w = info.width;
            memcpy(d.quant, info.quant, sizeof(d.quant));
            const size_t out_n = (size_t)info.width * info.height * 3;
            uint8_t *out = (uint8_t *)malloc(out_n);
            rc = ds_jpeg_reconstruct_host(coef, info.coef_count, &d, 1, out, (int64_t)out_n);
            free(out);
        }
        free(coef);
    }
    free(bytes);
    if (rc == DS_OK) ++g_ok; else ++g_unsupported;
    return rc;
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
        if (decode(data.data(), data.size()) != DS_OK) {
            fprintf(stderr, "%s: an intact file did not decode\n", path);
            return 2;
        }
        std::vector<uint8_t> m(data);
        for (int k = 0; k < mutations && !data.empty(); ++k) {
            const size_t at = next_u32() % data.size();
            const uint8_t keep = m[at];
            m[at] = (uint8_t)(keep ^ (1 + next_u32() % 255));
            decode(m.data(), m.size());
            m[at] = keep;
        }
        for (size_t cut = 0; cut <= (size_t)max_cut && cut < data.size(); ++cut) decode(data.data(), cut);
    }
    fclose(list);
    // the compiled tf.Example reader on the same damage: every prefix and seeded mutations of a small message
    {
        const uint8_t msg[] = {0x0a, 0x2b, 0x0a, 0x16, 0x0a, 0x0d, 'i', 'm', 'a', 'g', 'e', '/', 'e', 'n', 'c', 'o', 'd', 'e', 'd',
                               0x12, 0x05, 0x0a, 0x03, 0x0a, 0x01, 0x41, 0x0a, 0x11, 0x0a, 0x04, 't', 'e', 'x', 't', 0x12, 0x09,
                               0x1a, 0x07, 0x0a, 0x05, 0x03, 0x01, 0x04, 0x01, 0x05};
        int64_t text[50];
        ds_example_fields fields;
        for (size_t cut = 0; cut <= sizeof(msg); ++cut) {
            uint8_t *b = (uint8_t *)malloc(cut ? cut : 1);
            memcpy(b, msg, cut);
            ds_example_parse(b, (int64_t)cut, text, 50, &fields);
            free(b);
        }
        for (int k = 0; k < 20000; ++k) {
            uint8_t *b = (uint8_t *)malloc(sizeof(msg));
            memcpy(b, msg, sizeof(msg));
            b[next_u32() % sizeof(msg)] ^= (uint8_t)(1 + next_u32() % 255);
            if (ds_example_parse(b, (int64_t)sizeof(msg), text, 50, &fields) == DS_OK &&
                (fields.image_offset < 0 || fields.image_length < 0 || fields.image_offset + fields.image_length > (int64_t)sizeof(msg) ||
                 fields.text_len < 0 || fields.text_len > 50)) {
                free(b);
                return 3;
            }
            free(b);
        }
    }
    printf("files %ld decoded %ld rejected %ld\n", files, g_ok, g_unsupported);
    return 0;
}
