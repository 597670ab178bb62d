// ds_ragged_gather_host: the CPU statement of ds_ragged_gather (gather_bytes.hip), plain C++ on host pointers.  The
// usability test of a record and the place a destination byte comes from are gather_common.h's, shared with the kernel;
// what is left here is one loop that stores each destination byte of each usable window once.
#include <stdint.h>

#include "ds_kernels.h"
#include "gather_common.h"

extern "C" int ds_ragged_gather_host(const uint8_t *arena, int64_t narena, const uint8_t *spill, int64_t nspill,
                                     const ds_gather_desc *desc, int32_t batch, uint8_t *out, int64_t nout) {
    if (!arena || !desc || !out || narena < 0 || nspill < 0 || nout < 0 || batch < 1) return DS_ERR_ARG;
    if (!spill) nspill = 0;                        // a record that names an absent spill buffer fits nowhere
    for (int32_t i = 0; i < batch; ++i) {
        const ds_gather_desc d = desc[i];
        if (!dsgather::desc_ok(d, narena, nspill, nout)) continue;
        const uint8_t *src = (d.src ? spill : arena) + dsgather::window_origin(d);
        uint8_t *dst = out + d.out_offset;
        const uint32_t n = (uint32_t)dsgather::window_bytes(d);
        for (uint32_t k = 0; k < n; ++k) dst[k] = src[dsgather::source_byte(d, k)];
    }
    return DS_OK;
}
