// ds_ragged_gather: the batch assembly of the decoded-image cache.  One launch, blockIdx.y = image: a window of a resident
// packed-RGB uint8 image (arena or spill) is copied into the image's slot of the ragged batch buffer that
// ds_preprocess_eval / ds_preprocess_train read.  A pure byte mover with awkward alignment: pixels are 3 bytes and x0 is
// arbitrary, so source rows start at any byte; the destination window is ONE flat contiguous range whose start is
// 4-byte aligned and whose rows are not (3 * width is rarely a multiple of 4).
//
//   ragged_gather_kernel  the destination is walked as aligned 16-byte words.  A lane owns one word per turn and stores
//                         it as one global_store_dwordx4; consecutive lanes own consecutive words.  A word that lies in
//                         one source row (nearly all of them once 3 * width >= 32) is formed from five aligned source
//                         dwords -- one 4-byte-aligned dwordx4 load and one dword -- with four byte funnel shifts
//                         (v_alignbyte_b32); a word that straddles rows is formed dword by dword, each from two aligned
//                         dwords when its four bytes share a row and bytewise otherwise (width 1: a word holds pieces
//                         of six rows).  An aligned load that would reach past the end of the source buffer is not
//                         made: those last bytes are read bytewise.  The up-to-12 head bytes in front of the first
//                         aligned word and the up-to-15 tail bytes are stored bytewise by the image's first workgroup.
//                         Exactly one lane stores each destination byte; nothing else is written.  The address
//                         arithmetic and the usability test of a record are gather_common.h's, shared with the host
//                         statement (gather_host.cpp); a record that does not fit returns before any store.
#include "ds_common.h"
#include "gather_common.h"

namespace {

static_assert(sizeof(ds_gather_desc) == 40 && offsetof(ds_gather_desc, src_offset) == 0 && offsetof(ds_gather_desc, out_offset) == 8 &&
                  offsetof(ds_gather_desc, src) == 16 && offsetof(ds_gather_desc, pitch) == 20 && offsetof(ds_gather_desc, y0) == 24 &&
                  offsetof(ds_gather_desc, height) == 32 && offsetof(ds_gather_desc, width) == 36,
              "ds_gather_desc is ABI: ops.gather_desc_dtype() mirrors this layout");

struct __attribute__((packed, aligned(4))) dword4 {
    uint32_t a, b, c, d;
};

// destination bytes k .. k + 3 of the window (all inside it).  win: the window's first source byte; room: bytes from
// there to the end of the source buffer (the buffer's base is 4-byte aligned, so an aligned dword never starts before it)
__device__ __forceinline__ uint32_t gather_dword(const uint8_t *__restrict__ win, int64_t room, const ds_gather_desc &d,
                                                 uint32_t rowbytes, uint32_t k) {
    const uint32_t y = k / rowbytes, b = k - y * rowbytes;
    if (b + 4 <= rowbytes) {
        const int64_t rel = dsgather::row_byte(d, y, b);
        const uint8_t *p = win + rel;
        const uint32_t mis = (uint32_t)((uintptr_t)p & 3);
        if (rel - mis + 8 <= room) {
            const uint32_t *q = reinterpret_cast<const uint32_t *>(p - mis);
            return __builtin_amdgcn_alignbyte(q[1], q[0], mis);
        }
    }
    uint32_t v = 0;
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) v |= (uint32_t)win[dsgather::source_byte(d, k + j)] << (8 * j);
    return v;
}

__global__ __launch_bounds__(256) void ragged_gather_kernel(const uint8_t *__restrict__ arena, int64_t narena,
                                                            const uint8_t *__restrict__ spill, int64_t nspill,
                                                            const ds_gather_desc *__restrict__ desc, uint8_t *__restrict__ out,
                                                            int64_t nout) {
    const ds_gather_desc d = desc[blockIdx.y];
    if (!dsgather::desc_ok(d, narena, nspill, nout)) return;       // uniform over the workgroup: not a single store
    const int64_t origin = dsgather::window_origin(d);
    const uint8_t *win = (d.src ? spill : arena) + origin;
    const int64_t room = (d.src ? nspill : narena) - origin;
    uint8_t *dst = out + d.out_offset;
    const uint32_t n = (uint32_t)dsgather::window_bytes(d), rowbytes = (uint32_t)d.width * 3u;
    uint32_t head = (uint32_t)(-d.out_offset) & 15u;                // `out` is 16-byte aligned
    head = head < n ? head : n;
    const uint32_t words = (n - head) >> 4, tail = head + (words << 4);
    const uint32_t t = threadIdx.x;

    if (blockIdx.x == 0 && t < 32) {                               // lanes 0..15: the head, lanes 16..31: the tail
        const uint32_t k = t < 16 ? t : tail + (t - 16);
        if (t < 16 ? k < head : k < n) dst[k] = win[dsgather::source_byte(d, k)];
    }
    for (uint32_t i = blockIdx.x * 256u + t; i < words; i += gridDim.x * 256u) {
        const uint32_t k = head + (i << 4), y = k / rowbytes, b = k - y * rowbytes;
        uint4 v;
        bool wide = false;
        if (b + 16 <= rowbytes) {
            const int64_t rel = dsgather::row_byte(d, y, b);
            const uint8_t *p = win + rel;
            const uint32_t mis = (uint32_t)((uintptr_t)p & 3);
            if (rel - mis + 20 <= room) {
                const dword4 lo = *reinterpret_cast<const dword4 *>(p - mis);
                const uint32_t hi = *reinterpret_cast<const uint32_t *>(p - mis + 16);
                v.x = __builtin_amdgcn_alignbyte(lo.b, lo.a, mis);
                v.y = __builtin_amdgcn_alignbyte(lo.c, lo.b, mis);
                v.z = __builtin_amdgcn_alignbyte(lo.d, lo.c, mis);
                v.w = __builtin_amdgcn_alignbyte(hi, lo.d, mis);
                wide = true;
            }
        }
        if (!wide) {
            v.x = gather_dword(win, room, d, rowbytes, k);
            v.y = gather_dword(win, room, d, rowbytes, k + 4);
            v.z = gather_dword(win, room, d, rowbytes, k + 8);
            v.w = gather_dword(win, room, d, rowbytes, k + 12);
        }
        *reinterpret_cast<uint4 *>(dst + k) = v;
    }
}

}  // namespace

extern "C" int ds_ragged_gather(const uint8_t *arena, int64_t narena, const uint8_t *spill, int64_t nspill,
                                const ds_gather_desc *desc, int32_t batch, uint8_t *out, int64_t nout, void *stream) {
    DS_REQUIRE(arena && desc && out && narena >= 0 && nspill >= 0 && nout >= 0 && batch > 0, "ds_ragged_gather: bad argument");
    DS_REQUIRE(batch <= 65535, "ds_ragged_gather: at most 65535 images per launch");
    DS_REQUIRE(((uintptr_t)arena & 15) == 0 && ((uintptr_t)spill & 15) == 0 && ((uintptr_t)out & 15) == 0 && ((uintptr_t)desc & 7) == 0,
               "ds_ragged_gather: arena, spill and out must be 16-byte aligned, the table 8-byte");
    if (!spill) nspill = 0;                        // a record that names an absent spill buffer fits nowhere
    int gx = ds::kMaxStreamBlocks / batch;
    gx = gx < 1 ? 1 : gx > 64 ? 64 : gx;
    hipLaunchKernelGGL(ragged_gather_kernel, dim3(gx, batch), dim3(256), 0, (hipStream_t)stream, arena, narena, spill, nspill,
                       desc, out, nout);
    return ds::check_launch("ds_ragged_gather");
}
