// The sequential half of the JPEG decode, on the host: marker parse, Huffman decode into quantised coefficients, a
// compiled reader of one tf.train.Example payload, and the reconstruction in plain C++ (the CPU statement of what
// jpeg.hip computes; both use jpeg_common.h).  No HIP call, no global state, no allocation beyond a vector of restart
// segments and the planes of ds_jpeg_reconstruct_host; callable from any thread.  Contract: include/ds_kernels.h.
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

const uint8_t kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                             41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                             30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

constexpr int kLookBits = 9;
constexpr int64_t kMaxPixels = 89478485;       // Pillow's MAX_IMAGE_PIXELS: beyond it PIL warns or raises, so PIL decides

// What keeps the reconstruction equal to libjpeg-turbo's SIMD jpeg_idct_islow, which forms in0 + in4, in0 - in4, in7 + in3 and
// in5 + in1 in 16 bits in BOTH passes and packs the pass-1 workspace with saturation: a block is taken only when no pass-1
// output can leave +-16383, so that nothing wraps or saturates there and the 32-bit statement in jpeg_common.h is the same
// function.  A pass-1 output is 4 * sum_k w_k in_k over a column of dequantised coefficients with |w_0| = |w_4| = 1,
// |w_2|, |w_6| <= 1.30657 and |w_odd| <= 1.38704 (sqrt 2 cos); the test is sum_k ceil(4096 |w_k|) |in_k| <= 4090 * 4096 per
// column (4095.75 less the rounding of the 13-bit constants and of the descale).  Pixel data cannot come near it: by
// Parseval a column of an 8-bit block has sum_k |w_k| |F_k| <= 3.62 * 1024.
const int32_t kRowWeight[8] = {4096, 5682, 5352, 5682, 4096, 5682, 5352, 5682};
constexpr int32_t kColumnBound = 4090 * 4096;

struct Huffman {
    bool defined = false;
    uint8_t counts[17];            // codes of each length 1..16
    uint8_t vals[256];
    int nvals = 0;
    int32_t maxcode[18];           // largest code of length l, -1 when none
    int32_t valoff[17];            // vals index of the first code of length l, minus that code
    uint16_t look[1 << kLookBits]; // (length << 8) | symbol for codes of <= kLookBits bits, 0 otherwise
};

// derive the decoding tables; false when the counts do not describe a prefix code
bool build(Huffman &h, bool dc) {
    int32_t code = 0;
    int k = 0;
    memset(h.look, 0, sizeof(h.look));
    for (int l = 1; l <= 16; ++l) {
        h.valoff[l] = k - code;
        if (h.counts[l]) {
            if (code + h.counts[l] > (1 << l)) return false;
            for (int i = 0; i < h.counts[l]; ++i, ++k, ++code) {
                if (l <= kLookBits) {
                    const int first = code << (kLookBits - l);
                    for (int j = 0; j < (1 << (kLookBits - l)); ++j) h.look[first + j] = (uint16_t)((l << 8) | h.vals[k]);
                }
            }
            h.maxcode[l] = code - 1;
        } else {
            h.maxcode[l] = -1;
        }
        code <<= 1;
    }
    h.maxcode[17] = 0x7fffffff;
    if (dc)
        for (int i = 0; i < h.nvals; ++i)
            if (h.vals[i] > 15) return false;
    return true;
}

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
                h.counts[0] = 0;
                for (int l = 1; l <= 16; ++l) total += (h.counts[l] = p[o + l]);
                if (total > 256 || o + 17 + total > body) return false;
                memcpy(h.vals, p + o + 17, (size_t)total);
                h.nvals = total;
                if (!build(h, tc == 0)) return false;
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

// bits of one restart segment [p, end): inside it every 0xFF is followed by a stuffed 0x00 (walk_scan); past its end the
// reader supplies zeros and counts them
struct Bits {
    const uint8_t *p, *end;
    uint64_t acc = 0;
    int n = 0;                     // bits in acc (from the top)
    int fake = 0;                  // of which supplied past the end

    inline void refill() {
        while (n <= 56) {
            if (p < end) {
                const uint8_t v = *p++;
                if (v == 0xFF && p < end) ++p;
                acc |= (uint64_t)v << (56 - n);
            } else {
                fake += 8;
            }
            n += 8;
        }
    }
    inline uint32_t peek(int k) const { return (uint32_t)(acc >> (64 - k)); }
    inline void skip(int k) {
        acc <<= k;
        n -= k;
    }
    bool overrun() const { return n < fake; }
};

// one Huffman symbol, -1 when no code matches; at least 16 bits are in the buffer
inline int decode(Bits &br, const Huffman &h) {
    const uint16_t e = h.look[br.peek(kLookBits)];
    if (e) {
        br.skip(e >> 8);
        return e & 255;
    }
    for (int l = kLookBits + 1; l <= 16; ++l) {
        const int32_t code = (int32_t)br.peek(l);
        if (code <= h.maxcode[l]) {
            br.skip(l);
            return h.vals[(h.valoff[l] + code) & 255];
        }
    }
    return -1;
}

inline int receive_extend(Bits &br, int s) {
    const int v = (int)br.peek(s);
    br.skip(s);
    return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
}

// one block; false = unsupported
inline bool decode_block(Bits &br, const Huffman &dc, const Huffman &ac, const uint8_t *q, int &pred, int16_t *blk) {
    br.refill();
    int s = decode(br, dc);
    if (s < 0) return false;
    if (s) {
        br.refill();
        pred += receive_extend(br, s);
    }
    if (pred * (int)q[0] > 32767 || pred * (int)q[0] < -32767 || pred > 32767 || pred < -32767) return false;
    blk[0] = (int16_t)pred;
    int32_t column[8] = {0, 0, 0, 0, 0, 0, 0, 0};          // weighted |dequantised coefficient| per column: at most 8 * 32767 * 5682
    column[0] = kRowWeight[0] * (pred < 0 ? -pred : pred) * (int)q[0];
    for (int k = 1; k < 64;) {
        br.refill();
        const int rs = decode(br, ac);
        if (rs < 0) return false;
        const int r = rs >> 4;
        s = rs & 15;
        if (!s) {
            if (r != 15) break;                    // end of block
            k += 16;
            if (k > 64) return false;
            continue;
        }
        k += r;
        if (k > 63) return false;
        const int v = receive_extend(br, s);
        const int nat = kZigzag[k];
        const int prod = v * (int)q[nat];
        if (prod > 32767 || prod < -32767) return false;
        column[nat & 7] += kRowWeight[nat >> 3] * (prod < 0 ? -prod : prod);
        blk[nat] = (int16_t)v;
        ++k;
    }
    for (int c = 0; c < 8; ++c)
        if (column[c] > kColumnBound) return false;
    return !br.overrun();
}

int entropy_decode(const uint8_t *b, int64_t n, Header &hd, int16_t *coef) {
    std::vector<int64_t> cuts;
    if (!walk_scan(b, n, hd, &cuts)) return DS_JPEG_UNSUPPORTED;
    const dsjpeg::Geometry &g = hd.g;
    memset(coef, 0, (size_t)g.blocks * 128);
    const int mw = g.bw[hd.ncomp == 1 ? 0 : 1];
    const int bh[3] = {hd.ncomp == 1 ? 1 : g.hs, 1, 1}, bv[3] = {hd.ncomp == 1 ? 1 : g.vs, 1, 1};
    int64_t mcu = 0, begin = hd.scan_begin;
    for (size_t seg = 0; seg < cuts.size(); ++seg) {
        Bits br;
        br.p = b + begin;
        br.end = b + cuts[seg];
        int pred[3] = {0, 0, 0};
        const int64_t stop = hd.restart && mcu + hd.restart < hd.mcus ? mcu + hd.restart : hd.mcus;
        if (seg + 1 == cuts.size() && stop != hd.mcus) return DS_JPEG_UNSUPPORTED;
        for (; mcu < stop; ++mcu) {
            const int my = (int)(mcu / mw), mx = (int)(mcu % mw);
            for (int c = 0; c < hd.ncomp; ++c) {
                const Component &k = hd.comp[c];
                for (int v = 0; v < bv[c]; ++v)
                    for (int h = 0; h < bh[c]; ++h) {
                        const int64_t blk = g.base[c] + (int64_t)(my * bv[c] + v) * g.bw[c] + (mx * bh[c] + h);
                        if (!decode_block(br, hd.dc[k.td], hd.ac[k.ta], hd.q[k.tq], pred[c], coef + blk * 64))
                            return DS_JPEG_UNSUPPORTED;
                    }
            }
        }
        // the segment is used up: every byte fetched, less than a byte of padding left, no bit taken from past its end
        if (br.p != br.end || br.overrun() || br.n - br.fake >= 8) return DS_JPEG_UNSUPPORTED;
        begin = cuts[seg] + 2;
    }
    return mcu == hd.mcus ? DS_OK : DS_JPEG_UNSUPPORTED;
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
