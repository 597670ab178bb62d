// The sequential half of the JPEG decode, on the host: marker parse, Huffman decode into quantised coefficients, a
// compiled reader of one tf.train.Example payload, the reconstruction in plain C++ (the CPU statement of what jpeg.hip
// computes; both use jpeg_common.h), the scan description and host statement of the device Huffman decode, and the lossless
// restart transcoder.  No HIP call, no global state, no allocation beyond vectors of restart segments, the planes of
// ds_jpeg_reconstruct_host and the transcoder's coefficients and output; callable from any thread.  Contract:
// include/ds_kernels.h.
//
// The bytes are untrusted.  Every read goes through a position checked against the end of the buffer; every coefficient
// store is inside the image's block grid, whose size the caller's capacity was checked against.  Anything outside the
// supported set ends in DS_JPEG_UNSUPPORTED, never in a guess.
#include <stdint.h>
#include <string.h>
#include <vector>

#include "ds_kernels.h"
#include "jpeg_common.h"

namespace {

const uint8_t kZigzag[64] = DS_JPEG_ZIGZAG_INIT;

constexpr int64_t kMaxPixels = 89478485;       // Pillow's MAX_IMAGE_PIXELS: beyond it PIL warns or raises, so PIL decides

struct Huffman {
    bool defined = false;
    uint8_t counts[16];            // codes of each length 1..16: the DHT form, with vals
    uint8_t vals[256];
    int nvals = 0;
    dsjpeg::HuffTable t;           // the decoding tables (jpeg_common.h)
};

struct Component {
    int id, h, v, tq, td, ta;
};

struct Header {
    int width = 0, height = 0, ncomp = 0, sampling = -1, restart = 0;
    Component comp[3];
    bool qdefined[4] = {false, false, false, false};
    uint8_t q[4][64];              // natural order
    Huffman dc[4], ac[4];
    int64_t scan_begin = 0, scan_end = 0;      // entropy-coded bytes [begin, end); bytes[end], bytes[end + 1] = EOI
    dsjpeg::Geometry g;
    int64_t mcus = 0;
};

inline int be16(const uint8_t *p) { return (p[0] << 8) | p[1]; }

// markers up to and including SOS; false = unsupported
bool parse_header(const uint8_t *b, int64_t n, Header &hd) {
    if (n < 4 || b[0] != 0xFF || b[1] != 0xD8) return false;
    int64_t pos = 2;
    bool sof = false, adobe = false;
    int adobe_transform = -1;
    for (;;) {
        if (pos + 4 > n || b[pos] != 0xFF) return false;
        const int m = b[pos + 1];
        const int64_t len = be16(b + pos + 2);
        if (len < 2 || pos + 2 + len > n) return false;
        const uint8_t *p = b + pos + 4;
        const int64_t body = len - 2;
        pos += 2 + len;
        if (m == 0xDB) {                                               // DQT
            int64_t o = 0;
            while (o < body) {
                const int pq = p[o] >> 4, tq = p[o] & 15;
                if (pq != 0 || tq > 3 || o + 65 > body) return false;
                for (int i = 0; i < 64; ++i) hd.q[tq][kZigzag[i]] = p[o + 1 + i];
                hd.qdefined[tq] = true;
                o += 65;
            }
        } else if (m == 0xC4) {                                        // DHT
            int64_t o = 0;
            while (o < body) {
                if (o + 17 > body) return false;
                const int tc = p[o] >> 4, th = p[o] & 15;
                if (tc > 1 || th > 3) return false;
                Huffman &h = tc ? hd.ac[th] : hd.dc[th];
                int total = 0;
                for (int l = 1; l <= 16; ++l) total += (h.counts[l - 1] = p[o + l]);
                if (total > 256 || o + 17 + total > body) return false;
                memset(h.vals, 0, sizeof(h.vals));
                memcpy(h.vals, p + o + 17, (size_t)total);
                h.nvals = total;
                if (!dsjpeg::huff_build(h.counts, h.vals, tc == 0, h.t)) return false;
                h.defined = true;
                o += 17 + total;
            }
        } else if (m == 0xC0 || m == 0xC1) {                           // SOF0 / SOF1
            if (sof || body < 6) return false;
            sof = true;
            if (p[0] != 8) return false;
            hd.height = be16(p + 1);
            hd.width = be16(p + 3);
            hd.ncomp = p[5];
            if (hd.height < 1 || hd.width < 1 || (hd.ncomp != 1 && hd.ncomp != 3) || body != 6 + 3 * hd.ncomp) return false;
            for (int c = 0; c < hd.ncomp; ++c) {
                Component &k = hd.comp[c];
                k.id = p[6 + 3 * c];
                k.h = p[7 + 3 * c] >> 4;
                k.v = p[7 + 3 * c] & 15;
                k.tq = p[8 + 3 * c];
                if (k.h < 1 || k.h > 4 || k.v < 1 || k.v > 4 || k.tq > 3) return false;
            }
        } else if (m == 0xDD) {                                        // DRI
            if (body != 2) return false;
            hd.restart = be16(p);
        } else if (m == 0xEE) {                                        // APP14: Adobe
            if (body >= 12 && memcmp(p, "Adobe", 5) == 0) {
                adobe = true;
                adobe_transform = p[11];
            }
        } else if ((m >= 0xE0 && m <= 0xEF) || m == 0xFE) {            // other APPn, COM: skipped
        } else if (m == 0xDA) {                                        // SOS
            if (!sof || body != 4 + 2 * hd.ncomp || p[0] != hd.ncomp) return false;
            for (int c = 0; c < hd.ncomp; ++c) {
                Component &k = hd.comp[c];
                if (p[1 + 2 * c] != k.id) return false;              // the frame's order
                k.td = p[2 + 2 * c] >> 4;
                k.ta = p[2 + 2 * c] & 15;
                if (k.td > 3 || k.ta > 3 || !hd.dc[k.td].defined || !hd.ac[k.ta].defined || !hd.qdefined[k.tq]) return false;
            }
            const uint8_t *t = p + 1 + 2 * hd.ncomp;
            if (t[0] != 0 || t[1] != 63 || t[2] != 0) return false;    // Ss, Se, Ah/Al of a sequential scan
            hd.scan_begin = pos;
            break;
        } else {
            return false;             // progressive, arithmetic, lossless, hierarchical, DNL, RST / EOI / TEM out of place, ...
        }
    }
    if (hd.ncomp == 1) {
        hd.sampling = DS_JPEG_GREY;  // a single-component scan is not interleaved: its sampling factors do not matter
    } else {
        if (adobe && adobe_transform != 1) return false;
        if (hd.comp[0].id == 'R' && hd.comp[1].id == 'G' && hd.comp[2].id == 'B') return false;
        if (hd.comp[1].h != 1 || hd.comp[1].v != 1 || hd.comp[2].h != 1 || hd.comp[2].v != 1) return false;
        const int h = hd.comp[0].h, v = hd.comp[0].v;
        hd.sampling = h == 1 && v == 1 ? DS_JPEG_444 : h == 2 && v == 1 ? DS_JPEG_422 : h == 2 && v == 2 ? DS_JPEG_420 : -1;
        if (hd.sampling < 0) return false;
    }
    if ((int64_t)hd.width * hd.height > kMaxPixels) return false;
    if (!dsjpeg::geometry(hd.width, hd.height, hd.sampling, hd.g)) return false;
    hd.mcus = (int64_t)hd.g.bw[hd.ncomp == 1 ? 0 : 1] * hd.g.bh[hd.ncomp == 1 ? 0 : 1];
    return true;
}

// walk the entropy-coded bytes: 0xFF is followed by 0x00, by the next restart marker in sequence, or by EOI; `cuts`
// receives the end of every restart segment (the position of its marker)
bool walk_scan(const uint8_t *b, int64_t n, Header &hd, std::vector<int64_t> *cuts) {
    const int64_t intervals = hd.restart ? (hd.mcus + hd.restart - 1) / hd.restart : 1;
    int64_t pos = hd.scan_begin, seen = 0;
    for (;;) {
        if (pos >= n) return false;
        const uint8_t *f = (const uint8_t *)memchr(b + pos, 0xFF, (size_t)(n - pos));
        if (!f) return false;
        pos = f - b;
        if (pos + 1 >= n) return false;
        const int m = b[pos + 1];
        if (m == 0x00) {
            pos += 2;
        } else if (m >= 0xD0 && m <= 0xD7) {
            if (!hd.restart || seen + 1 >= intervals || m != 0xD0 + (int)(seen & 7)) return false;
            if (cuts) cuts->push_back(pos);
            ++seen;
            pos += 2;
        } else if (m == 0xD9) {
            if (seen + 1 != intervals) return false;
            if (cuts) cuts->push_back(pos);
            hd.scan_end = pos;
            // a block takes at least two bits (a DC code and an end-of-block code): a header that claims more blocks than
            // the scan can hold is rejected here, before anybody sizes or touches storage for it
            return hd.g.blocks <= (pos - hd.scan_begin) * 4;
        } else {
            return false;
        }
    }
}

void fill_info(const Header &hd, ds_jpeg_info *info) {
    info->width = hd.width;
    info->height = hd.height;
    info->components = hd.ncomp;
    info->sampling = hd.sampling;
    info->restart_interval = hd.restart;
    info->supported = 1;
    info->coef_count = hd.g.blocks * 64;
    info->coef_bytes = hd.g.blocks * 128;
    for (int c = 0; c < hd.ncomp; ++c) memcpy(info->quant[c], hd.q[hd.comp[c].tq], 64);
}

// the tables a segment decode reads, from the header
dsjpeg::SegmentTables segment_tables(const Header &hd) {
    dsjpeg::SegmentTables t = {};
    for (int c = 0; c < hd.ncomp; ++c) {
        t.dc[c] = &hd.dc[hd.comp[c].td].t;
        t.ac[c] = &hd.ac[hd.comp[c].ta].t;
        t.q[c] = hd.q[hd.comp[c].tq];
    }
    t.zigzag = kZigzag;
    return t;
}

int entropy_decode(const uint8_t *b, int64_t n, Header &hd, int16_t *coef) {
    std::vector<int64_t> cuts;
    if (!walk_scan(b, n, hd, &cuts)) return DS_JPEG_UNSUPPORTED;
    memset(coef, 0, (size_t)hd.g.blocks * 128);
    const dsjpeg::SegmentTables t = segment_tables(hd);
    int64_t mcu = 0, begin = hd.scan_begin;
    for (size_t seg = 0; seg < cuts.size(); ++seg) {
        const int64_t stop = hd.restart && mcu + hd.restart < hd.mcus ? mcu + hd.restart : hd.mcus;
        if (seg + 1 == cuts.size() && stop != hd.mcus) return DS_JPEG_UNSUPPORTED;
        int32_t column[8];
        if (dsjpeg::decode_segment(b + begin, b + cuts[seg], mcu, stop - mcu, hd.g, t, coef, column, 1)) return DS_JPEG_UNSUPPORTED;
        mcu = stop;
        begin = cuts[seg] + 2;
    }
    return mcu == hd.mcus ? DS_OK : DS_JPEG_UNSUPPORTED;
}

void fill_scan(const Header &hd, const std::vector<int64_t> &cuts, ds_jpeg_scan_info *scan) {
    memset(scan, 0, sizeof(*scan));
    scan->scan_begin = hd.scan_begin;
    scan->cut_count = (int64_t)cuts.size();
    for (int c = 0; c < hd.ncomp; ++c) {
        const Huffman &dc = hd.dc[hd.comp[c].td], &ac = hd.ac[hd.comp[c].ta];
        memcpy(scan->dc[c].counts, dc.counts, 16);
        memcpy(scan->dc[c].values, dc.vals, 256);
        memcpy(scan->ac[c].counts, ac.counts, 16);
        memcpy(scan->ac[c].values, ac.vals, 256);
    }
}

// info, scan and (when they fit) the cuts of a stream
int scan_stream(const uint8_t *bytes, int64_t n, ds_jpeg_info *info, ds_jpeg_scan_info *scan, int64_t *cuts, int64_t capacity) {
    memset(info, 0, sizeof(*info));
    info->sampling = -1;
    memset(scan, 0, sizeof(*scan));
    Header hd;
    std::vector<int64_t> found;
    if (!parse_header(bytes, n, hd) || !walk_scan(bytes, n, hd, &found)) return DS_JPEG_UNSUPPORTED;
    fill_info(hd, info);
    fill_scan(hd, found, scan);
    if ((int64_t)found.size() > capacity) return DS_JPEG_MORE;
    memcpy(cuts, found.data(), found.size() * sizeof(int64_t));
    return DS_OK;
}

// ---- restart transcoder --------------------------------------------------------------------------------------------------------
// The typical Huffman tables of Annex K of the JPEG standard (K.3 - K.6), in DHT form: what a table that lacks a needed
// symbol is replaced by.  Every DC category 0..11 and every AC symbol run 0..15 x size 1..10, EOB and ZRL has a code.
struct StdTable {
    uint8_t counts[16];
    int nvals;
    const uint8_t *vals;
};
const uint8_t kStdDcVals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
const uint8_t kStdAcLumaVals[162] = {
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81,
    0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18,
    0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
    0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75,
    0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99,
    0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
    0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5,
    0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};
const uint8_t kStdAcChromaVals[162] = {
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08,
    0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25,
    0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47,
    0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74,
    0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97,
    0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
    0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4,
    0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};
const StdTable kStdTables[2][2] = {          // [class: DC, AC][luma, chroma]
    {{{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, 12, kStdDcVals}, {{0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}, 12, kStdDcVals}},
    {{{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125}, 162, kStdAcLumaVals},
     {{0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119}, 162, kStdAcChromaVals}}};

// the encoder's view of a table: code and length per symbol (length 0 = the table has no code for it)
struct Encoder {
    uint16_t code[256];
    uint8_t size[256];
};

void make_encoder(const Huffman &h, Encoder &e) {
    memset(&e, 0, sizeof(e));
    uint32_t code = 0;
    int k = 0;
    for (int l = 1; l <= 16; ++l) {
        for (int i = 0; i < h.counts[l - 1]; ++i, ++k, ++code)
            if (!e.size[h.vals[k]]) {          // (a repeated value keeps its first code)
                e.code[h.vals[k]] = (uint16_t)code;
                e.size[h.vals[k]] = (uint8_t)l;
            }
        code <<= 1;
    }
}

inline int bit_length(int v) {                 // of |v| <= 65534
    v = v < 0 ? -v : v;
    int s = 0;
    while (v) {
        ++s;
        v >>= 1;
    }
    return s;
}

// The blocks of the image in scan order with the DC predictors reset every `interval` MCUs: `use` sees every symbol,
// use(table class, component, symbol, extra bits, their count); restart(index) runs between two intervals.
template <class Use, class Restart>
void for_each_symbol(const Header &hd, const int16_t *coef, int64_t interval, Use use, Restart restart) {
    const dsjpeg::Geometry &g = hd.g;
    const int mw = g.bw[hd.ncomp == 1 ? 0 : 1];
    int pred[3] = {0, 0, 0};
    for (int64_t mcu = 0; mcu < hd.mcus; ++mcu) {
        if (mcu && mcu % interval == 0) {
            restart(mcu / interval - 1);
            pred[0] = pred[1] = pred[2] = 0;
        }
        const int my = (int)(mcu / mw), mx = (int)(mcu % mw);
        for (int c = 0; c < hd.ncomp; ++c) {
            const int bh = c == 0 ? g.hs : 1, bv = c == 0 ? g.vs : 1;
            for (int v = 0; v < bv; ++v)
                for (int h = 0; h < bh; ++h) {
                    const int16_t *blk = coef + (g.base[c] + (int64_t)(my * bv + v) * g.bw[c] + (mx * bh + h)) * 64;
                    const int diff = blk[0] - pred[c];
                    pred[c] = blk[0];
                    int s = bit_length(diff);
                    use(0, c, s, (uint32_t)(diff < 0 ? diff - 1 : diff) & ((1u << s) - 1), s);
                    int run = 0;
                    for (int k = 1; k < 64; ++k) {
                        const int x = blk[kZigzag[k]];
                        if (!x) {
                            ++run;
                            continue;
                        }
                        for (; run > 15; run -= 16) use(1, c, 0xF0, 0, 0);
                        s = bit_length(x);
                        use(1, c, (run << 4) | s, (uint32_t)(x < 0 ? x - 1 : x) & ((1u << s) - 1), s);
                        run = 0;
                    }
                    if (run) use(1, c, 0x00, 0, 0);
                }
        }
    }
}

// entropy-coded bytes: bits from the top, a stuffed 0x00 behind every 0xFF
struct BitWriter {
    std::vector<uint8_t> &out;
    uint32_t acc = 0;
    int n = 0;
    explicit BitWriter(std::vector<uint8_t> &o) : out(o) {}
    void put(uint32_t bits, int count) {       // count <= 16
        acc = (acc << count) | bits;
        n += count;
        while (n >= 8) {
            const uint8_t v = (uint8_t)(acc >> (n - 8));
            out.push_back(v);
            if (v == 0xFF) out.push_back(0x00);
            n -= 8;
        }
        acc &= (1u << n) - 1;
    }
    void pad() {                               // one-bits up to the byte boundary
        if (n) put((1u << (8 - n)) - 1, 8 - n);
    }
};

int restart_transcode(const uint8_t *b, int64_t n, int32_t interval_mcus, std::vector<uint8_t> &out) {
    Header hd;
    if (!parse_header(b, n, hd)) return DS_JPEG_UNSUPPORTED;
    std::vector<int16_t> coef((size_t)hd.g.blocks * 64);
    if (entropy_decode(b, n, hd, coef.data()) != DS_OK) return DS_JPEG_UNSUPPORTED;
    const int64_t interval = interval_mcus ? interval_mcus : hd.g.bw[hd.ncomp == 1 ? 0 : 1];       // a row: <= 8192 MCUs
    // the symbols the new stream needs, per table; a table that lacks one is replaced by its class's Annex K table
    bool need[2][4][256] = {};
    bool wide = false;
    for_each_symbol(hd, coef.data(), interval,
                    [&](int cls, int c, int sym, uint32_t, int s) {
                        need[cls][cls ? hd.comp[c].ta : hd.comp[c].td][sym] = true;
                        wide |= s > 15;
                    },
                    [](int64_t) {});
    if (wide) return DS_JPEG_UNSUPPORTED;      // (a DC difference of 17 bits: between predictors of opposite extremes)
    Encoder enc[2][4];
    for (int cls = 0; cls < 2; ++cls)
        for (int id = 0; id < 4; ++id) {
            Huffman &h = cls ? hd.ac[id] : hd.dc[id];
            if (!h.defined) continue;
            make_encoder(h, enc[cls][id]);
            bool missing = false;
            for (int sym = 0; sym < 256; ++sym) missing |= need[cls][id][sym] && !enc[cls][id].size[sym];
            if (!missing) continue;
            bool luma = false;
            for (int c = 0; c < hd.ncomp; ++c) luma |= c == 0 && (cls ? hd.comp[c].ta : hd.comp[c].td) == id;
            const StdTable &st = kStdTables[cls][luma ? 0 : 1];
            memcpy(h.counts, st.counts, 16);
            memset(h.vals, 0, sizeof(h.vals));
            memcpy(h.vals, st.vals, (size_t)st.nvals);
            h.nvals = st.nvals;
            make_encoder(h, enc[cls][id]);
            for (int sym = 0; sym < 256; ++sym)
                if (need[cls][id][sym] && !enc[cls][id].size[sym]) return DS_JPEG_UNSUPPORTED;
        }
    // the segments in front of the scan: everything but DRI and DHT as it is; then the tables, the interval and SOS
    out.clear();
    out.reserve((size_t)n + (size_t)n / 8 + 1024);
    out.push_back(0xFF);
    out.push_back(0xD8);
    int64_t pos = 2, sos = 0;
    for (;;) {                                 // parse_header accepted these bytes: every length is inside the buffer
        const int m = b[pos + 1];
        const int64_t len = be16(b + pos + 2);
        if (m == 0xDA) {
            sos = pos;
            break;
        }
        if (m != 0xDD && m != 0xC4) out.insert(out.end(), b + pos, b + pos + 2 + len);
        pos += 2 + len;
    }
    size_t dht = 2;
    for (int cls = 0; cls < 2; ++cls)
        for (int id = 0; id < 4; ++id)
            if ((cls ? hd.ac[id] : hd.dc[id]).defined) dht += 17 + (size_t)(cls ? hd.ac[id] : hd.dc[id]).nvals;
    if (dht > 65535) return DS_JPEG_UNSUPPORTED;
    out.push_back(0xFF);
    out.push_back(0xC4);
    out.push_back((uint8_t)(dht >> 8));
    out.push_back((uint8_t)dht);
    for (int cls = 0; cls < 2; ++cls)
        for (int id = 0; id < 4; ++id) {
            const Huffman &h = cls ? hd.ac[id] : hd.dc[id];
            if (!h.defined) continue;
            out.push_back((uint8_t)((cls << 4) | id));
            out.insert(out.end(), h.counts, h.counts + 16);
            out.insert(out.end(), h.vals, h.vals + h.nvals);
        }
    const uint8_t dri[6] = {0xFF, 0xDD, 0x00, 0x04, (uint8_t)(interval >> 8), (uint8_t)interval};
    out.insert(out.end(), dri, dri + 6);
    out.insert(out.end(), b + sos, b + hd.scan_begin);
    BitWriter w(out);
    for_each_symbol(hd, coef.data(), interval,
                    [&](int cls, int c, int sym, uint32_t extra, int s) {
                        const Encoder &e = enc[cls][cls ? hd.comp[c].ta : hd.comp[c].td];
                        w.put(e.code[sym], e.size[sym]);
                        if (s) w.put(extra, s);
                    },
                    [&](int64_t index) {
                        w.pad();
                        out.push_back(0xFF);
                        out.push_back((uint8_t)(0xD0 + (index & 7)));
                    });
    w.pad();
    out.insert(out.end(), b + hd.scan_end, b + n);           // EOI and whatever follows it
    return DS_OK;
}

// ---- tf.train.Example ------------------------------------------------------------------------------------------------------
struct Span {
    const uint8_t *p;
    int64_t n;
};

// protobuf field iterator over a span; next() = 1 (a field), 0 (end), -1 (malformed)
struct Fields {
    const uint8_t *p, *end;
    int field = 0, wt = 0;
    uint64_t val = 0;              // wire type 0
    Span bytes = {nullptr, 0};     // wire types 2, 1, 5

    explicit Fields(Span s) : p(s.p), end(s.p + s.n) {}

    bool varint(uint64_t &out) {
        uint64_t r = 0;
        for (int shift = 0; shift < 70; shift += 7) {
            if (p >= end) return false;
            const uint8_t v = *p++;
            if (shift == 63 && (v & 0x7E)) return false;          // beyond 64 bits
            r |= (uint64_t)(v & 0x7F) << (shift < 64 ? shift : 63);
            if (!(v & 0x80)) {
                out = r;
                return true;
            }
        }
        return false;
    }

    int next() {
        if (p >= end) return 0;
        uint64_t key;
        if (!varint(key) || (key >> 3) > 0x1FFFFFFF) return -1;
        field = (int)(key >> 3);
        wt = (int)(key & 7);
        if (wt == 0) return varint(val) ? 1 : -1;
        uint64_t len = wt == 5 ? 4 : 8;
        if (wt == 2) {
            if (!varint(len)) return -1;
        } else if (wt != 1 && wt != 5) {
            return -1;
        }
        if (len > (uint64_t)(end - p)) return -1;
        bytes = {p, (int64_t)len};
        p += len;
        return 1;
    }
};

enum Key { kNone, kImage, kText, kSeqLen, kLabel, kPostId, kDay };

Key classify(Span k) {
    static const struct {
        const char *name;
        Key key;
    } names[] = {{"image/encoded", kImage}, {"text", kText},       {"seq_len", kSeqLen},
                 {"image/class/label", kLabel}, {"post_id", kPostId}, {"day", kDay}};
    for (const auto &e : names)
        if ((int64_t)strlen(e.name) == k.n && memcmp(e.name, k.p, (size_t)k.n) == 0) return e.key;
    return kNone;
}

// the int64 values of a Feature into out[0 .. cap); returns how many there are (-1 = not taken)
int64_t int_values(Span feat, int64_t *out, int64_t cap) {
    int64_t count = 0;
    Fields f(feat);
    int r;
    while ((r = f.next()) == 1) {
        if (f.field < 1 || f.field > 3 || f.wt != 2) continue;    // unknown fields are skipped
        if (f.field != 3) return -1;                              // a bytes or float list under an integer key
        Fields l(f.bytes);
        int rl;
        while ((rl = l.next()) == 1) {
            if (l.field != 1) continue;
            if (l.wt == 0) {
                if (count < cap) out[count] = (int64_t)l.val;
                ++count;
            } else if (l.wt == 2) {
                Fields v(l.bytes);
                while (v.p < v.end) {
                    uint64_t x;
                    if (!v.varint(x)) return -1;
                    if (count < cap) out[count] = (int64_t)x;
                    ++count;
                }
            } else {
                return -1;
            }
        }
        if (rl < 0) return -1;
    }
    return r < 0 ? -1 : count;
}

}  // namespace

extern "C" int ds_example_parse(const uint8_t *rec, int64_t n, int64_t *text, int32_t text_capacity,
                                ds_example_fields *out) {
    if (!rec || n < 0 || !text || text_capacity < 0 || !out) return DS_ERR_ARG;
    memset(out, 0, sizeof(*out));
    out->image_length = -1;
    int64_t *const ints[4] = {&out->seq_len, &out->label, &out->post_id, &out->day};
    Fields top(Span{rec, n});
    int r1;
    while ((r1 = top.next()) == 1) {
        if (top.field != 1 || top.wt != 2) continue;
        Fields feats(top.bytes);
        int r2;
        while ((r2 = feats.next()) == 1) {
            if (feats.field != 1 || feats.wt != 2) continue;
            Span key = {nullptr, -1}, feat = {nullptr, 0};
            Fields e(feats.bytes);
            int r3;
            while ((r3 = e.next()) == 1) {
                if (e.field != 1 && e.field != 2) continue;
                if (e.wt != 2) return DS_JPEG_UNSUPPORTED;
                (e.field == 1 ? key : feat) = e.bytes;
            }
            if (r3 < 0 || key.n < 0) return DS_JPEG_UNSUPPORTED;
            for (int64_t i = 0; i < key.n; ++i)
                if (key.p[i] & 0x80) return DS_JPEG_UNSUPPORTED;     // the Python parser decodes keys as UTF-8
            const Key k = classify(key);
            if (k == kNone) {                                        // still has to be well formed for the Python parser
                Fields f(feat);
                int r;
                while ((r = f.next()) == 1) {
                    if (f.field < 1 || f.field > 3 || f.wt != 2) continue;
                    Fields l(f.bytes);
                    int rl;
                    while ((rl = l.next()) == 1) {
                    }
                    if (rl < 0) return DS_JPEG_UNSUPPORTED;
                }
                if (r < 0) return DS_JPEG_UNSUPPORTED;
            } else if (k == kImage) {
                out->image_length = -1;
                Fields f(feat);
                int r;
                while ((r = f.next()) == 1) {
                    if (f.field < 1 || f.field > 3 || f.wt != 2) continue;
                    if (f.field != 1) return DS_JPEG_UNSUPPORTED;
                    Fields l(f.bytes);
                    int rl;
                    while ((rl = l.next()) == 1) {
                        if (l.field != 1) continue;
                        if (l.wt != 2) return DS_JPEG_UNSUPPORTED;
                        if (out->image_length < 0) {
                            out->image_offset = l.bytes.p - rec;
                            out->image_length = l.bytes.n;
                        }
                    }
                    if (rl < 0) return DS_JPEG_UNSUPPORTED;
                }
                if (r < 0) return DS_JPEG_UNSUPPORTED;
            } else if (k == kText) {
                const int64_t c = int_values(feat, text, text_capacity);
                if (c < 0 || c > text_capacity) return DS_JPEG_UNSUPPORTED;
                out->text_len = (int32_t)c;
                for (int64_t i = c; i < text_capacity; ++i) text[i] = 0;        // a repeated key: the last list wins, whole
            } else {
                int64_t first = 0;
                if (int_values(feat, &first, 1) < 1) return DS_JPEG_UNSUPPORTED;      // an empty list: the Python parser raises
                *ints[k - kSeqLen] = first;
            }
        }
        if (r2 < 0) return DS_JPEG_UNSUPPORTED;
    }
    if (r1 < 0 || out->image_length < 0) return DS_JPEG_UNSUPPORTED;
    return DS_OK;
}

extern "C" int ds_jpeg_probe(const uint8_t *bytes, int64_t n, ds_jpeg_info *info) {
    if (!bytes || n < 0 || !info) return DS_ERR_ARG;
    memset(info, 0, sizeof(*info));
    info->sampling = -1;
    Header hd;
    if (!parse_header(bytes, n, hd) || !walk_scan(bytes, n, hd, nullptr)) return DS_JPEG_UNSUPPORTED;
    fill_info(hd, info);
    return DS_OK;
}

extern "C" int ds_jpeg_entropy_decode(const uint8_t *bytes, int64_t n, const ds_jpeg_info *info, int16_t *coef,
                                      int64_t capacity) {
    if (!bytes || n < 0 || !info || !coef || capacity < 0) return DS_ERR_ARG;
    Header hd;
    if (!parse_header(bytes, n, hd)) return DS_JPEG_UNSUPPORTED;
    // `info` must be this stream's: the sizes below come from the bytes, never from the caller
    if (!info->supported || info->width != hd.width || info->height != hd.height || info->sampling != hd.sampling ||
        info->coef_count != hd.g.blocks * 64)
        return DS_ERR_ARG;
    if (capacity < hd.g.blocks * 64) return DS_JPEG_MORE;
    return entropy_decode(bytes, n, hd, coef);
}

extern "C" int ds_jpeg_record_decode(const uint8_t *rec, int64_t n, int64_t *text, int32_t text_capacity,
                                     ds_example_fields *fields, ds_jpeg_info *info, int16_t *coef, int64_t capacity,
                                     int32_t *jpeg_status) {
    if (!info || !jpeg_status || capacity < 0 || (capacity > 0 && !coef)) return DS_ERR_ARG;
    const int rc = ds_example_parse(rec, n, text, text_capacity, fields);
    if (rc != DS_OK) return rc;
    memset(info, 0, sizeof(*info));
    info->sampling = -1;
    *jpeg_status = DS_JPEG_UNSUPPORTED;
    const uint8_t *bytes = rec + fields->image_offset;
    const int64_t nb = fields->image_length;
    Header hd;
    if (!parse_header(bytes, nb, hd)) return DS_OK;
    if (capacity < hd.g.blocks * 64) {
        if (!walk_scan(bytes, nb, hd, nullptr)) return DS_OK;
        fill_info(hd, info);
        *jpeg_status = DS_JPEG_MORE;
        return DS_OK;
    }
    if (entropy_decode(bytes, nb, hd, coef) != DS_OK) return DS_OK;
    fill_info(hd, info);
    *jpeg_status = DS_OK;
    return DS_OK;
}

extern "C" int ds_jpeg_reconstruct_host(const int16_t *coef, int64_t ncoef, const ds_jpeg_desc *desc, int32_t batch,
                                        uint8_t *out_bytes, int64_t nbytes) {
    if (!coef || !desc || !out_bytes || ncoef < 0 || nbytes < 0 || batch < 1) return DS_ERR_ARG;
    std::vector<uint8_t> planes;
    for (int32_t b = 0; b < batch; ++b) {
        const ds_jpeg_desc &d = desc[b];
        dsjpeg::Geometry g;
        if (!dsjpeg::geometry(d.width, d.height, d.sampling, g)) return DS_ERR_ARG;
        if (d.coef_offset < 0 || d.coef_offset > ncoef || g.blocks * 64 > ncoef - d.coef_offset) return DS_ERR_ARG;
        if (d.y0 < 0 || d.x0 < 0 || d.crop_h < 1 || d.crop_w < 1 || d.crop_h > d.height - d.y0 || d.crop_w > d.width - d.x0)
            return DS_ERR_ARG;
        const int64_t out_n = (int64_t)d.crop_h * d.crop_w * 3;
        if (d.out_offset < 0 || d.out_offset > nbytes || out_n > nbytes - d.out_offset) return DS_ERR_ARG;
        planes.assign((size_t)g.blocks * 64, 0);
        for (int c = 0; c < g.ncomp; ++c) {
            const int pitch = g.bw[c] * 8;
            for (int by = 0; by < g.bh[c]; ++by)
                for (int bx = 0; bx < g.bw[c]; ++bx) {
                    const int16_t *blk = coef + d.coef_offset + (g.base[c] + (int64_t)by * g.bw[c] + bx) * 64;
                    int32_t ws[64];
                    for (int col = 0; col < 8; ++col) {
                        int32_t in[8], o[8];
                        for (int r = 0; r < 8; ++r) in[r] = (int32_t)blk[r * 8 + col] * (int32_t)d.quant[c][r * 8 + col];
                        dsjpeg::idct_column(in, o);
                        for (int r = 0; r < 8; ++r) ws[r * 8 + col] = o[r];
                    }
                    uint8_t *dst = planes.data() + g.base[c] * 64 + (int64_t)by * 8 * pitch + bx * 8;
                    for (int r = 0; r < 8; ++r) {
                        int32_t o[8];
                        dsjpeg::idct_row(ws + r * 8, o);
                        for (int col = 0; col < 8; ++col) dst[(int64_t)r * pitch + col] = (uint8_t)o[col];
                    }
                }
        }
        dsjpeg::Plane pl[3];
        dsjpeg::planes_of(planes.data(), g, pl);
        uint8_t *dst = out_bytes + d.out_offset;
        for (int y = 0; y < d.crop_h; ++y)
            for (int x = 0; x < d.crop_w; ++x, dst += 3) dsjpeg::pixel(pl, g, d.y0 + y, d.x0 + x, dst);
    }
    return DS_OK;
}

extern "C" int ds_jpeg_scan(const uint8_t *bytes, int64_t n, ds_jpeg_info *info, ds_jpeg_scan_info *scan, int64_t *cuts,
                            int64_t capacity) {
    if (!bytes || n < 0 || !info || !scan || capacity < 0 || (capacity > 0 && !cuts)) return DS_ERR_ARG;
    return scan_stream(bytes, n, info, scan, cuts, capacity);
}

extern "C" int ds_jpeg_record_scan(const uint8_t *rec, int64_t n, int64_t *text, int32_t text_capacity, ds_example_fields *fields,
                                   ds_jpeg_info *info, ds_jpeg_scan_info *scan, int64_t *cuts, int64_t capacity,
                                   int32_t *jpeg_status) {
    if (!info || !scan || !jpeg_status || capacity < 0 || (capacity > 0 && !cuts)) return DS_ERR_ARG;
    const int rc = ds_example_parse(rec, n, text, text_capacity, fields);
    if (rc != DS_OK) return rc;
    *jpeg_status = scan_stream(rec + fields->image_offset, fields->image_length, info, scan, cuts, capacity);
    return DS_OK;
}

extern "C" int ds_jpeg_restart_transcode(const uint8_t *bytes, int64_t n, int32_t interval_mcus, uint8_t *out, int64_t capacity,
                                         int64_t *out_n) {
    if (!bytes || n < 0 || interval_mcus < 0 || interval_mcus > 65535 || capacity < 0 || (capacity > 0 && !out) || !out_n)
        return DS_ERR_ARG;
    *out_n = 0;
    std::vector<uint8_t> stream;
    const int rc = restart_transcode(bytes, n, interval_mcus, stream);
    if (rc != DS_OK) return rc;
    *out_n = (int64_t)stream.size();
    if (capacity < *out_n) return DS_JPEG_MORE;
    memcpy(out, stream.data(), stream.size());
    return DS_OK;
}

extern "C" int ds_jpeg_entropy_decode_segments_host(const uint8_t *scan, int64_t nscan, const ds_jpeg_scan_desc *images,
                                                    int32_t nimages, const ds_jpeg_segment *segs, int64_t nsegs, int16_t *coef,
                                                    int64_t ncoef, int32_t *status) {
    if (!scan || nscan < 0 || !images || nimages < 1 || !segs || nsegs < 0 || !coef || ncoef < 0 || !status) return DS_ERR_ARG;
    std::vector<dsjpeg::HuffTable> tables(6);
    for (int32_t b = 0; b < nimages; ++b) {
        const ds_jpeg_scan_desc &d = images[b];
        status[b] = DS_JPEG_E_TABLE;
        dsjpeg::Geometry g;
        if (!dsjpeg::scan_desc_ok(d, ncoef, nsegs, g)) continue;
        dsjpeg::SegmentTables t = {};
        bool ok = true;
        for (int c = 0; c < g.ncomp; ++c) {
            ok = ok && dsjpeg::huff_build(d.dc[c].counts, d.dc[c].values, true, tables[c]);
            ok = ok && dsjpeg::huff_build(d.ac[c].counts, d.ac[c].values, false, tables[3 + c]);
            t.dc[c] = &tables[c];
            t.ac[c] = &tables[3 + c];
            t.q[c] = d.quant[c];
        }
        t.zigzag = kZigzag;
        if (!ok) continue;
        int16_t *image = coef + d.coef_offset;
        memset(image, 0, (size_t)g.blocks * 128);
        int err = 0;
        const ds_jpeg_segment *sg = segs + d.first_segment;
        for (int i = 0; i < d.segments; ++i) {
            if (!dsjpeg::segment_ok(sg[i], sg[i ? i - 1 : 0], i, d.segments, nscan, dsjpeg::mcu_count(g))) {
                err |= DS_JPEG_E_TABLE;
                continue;
            }
            int32_t column[8];
            err |= dsjpeg::decode_segment(scan + sg[i].begin, scan + sg[i].end, sg[i].first_mcu, sg[i].mcus, g, t, image, column, 1);
        }
        status[b] = err;
    }
    return DS_OK;
}
