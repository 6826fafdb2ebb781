// d2d_segments_host.cpp -- the CPU twins of the segment calls (include/dsd2dxd_amd.h, "A chunk's bookkeeping in one launch"): the
// checks of d2d_segments_internal.h and memcpy.  No HIP: tools/segments_fuzz.cpp and the CPU tests build on this file with g++ alone.
#include <string.h>

#include "d2d_segments_internal.h"

using namespace d2dseg;

extern "C" {

int d2d_segments_move_host(const d2d_segment* seg, uint32_t n) {
    const int rc = check_move(seg, n);
    if (rc != D2D_OK) return rc;
    for (uint32_t i = 0; i < n; ++i)
        if (seg[i].bytes) memcpy(seg[i].dst, seg[i].src, seg[i].bytes);
    return D2D_OK;
}

int d2d_segments_pack_host(const d2d_pack_src* src, uint32_t n, void* dst, size_t dst_capacity, uint64_t* offsets) {
    const int rc = check_pack(src, n, dst, dst_capacity, offsets, 1);
    if (rc != D2D_OK) return rc;
    auto put = [&](uint32_t k, uint64_t v) { memcpy((uint8_t*)offsets + (size_t)k * 8, &v, 8); };       // (the table needs no alignment here)
    bool fits = true;
    std::vector<uint64_t> len(n);
    for (uint32_t k = 0; k < n; ++k) {
        memcpy(&len[k], src[k].bytes, 8);
        if (len[k] > src[k].max_bytes) fits = false;
    }
    if (!fits) {
        for (uint32_t k = 0; k <= n; ++k) put(k, UINT64_MAX);
        return D2D_OK;
    }
    uint64_t off = 0;
    for (uint32_t k = 0; k < n; ++k) {
        put(k, off);
        if (len[k]) memcpy((uint8_t*)dst + off, src[k].base, (size_t)len[k]);
        off += len[k];
    }
    put(n, off);
    return D2D_OK;
}

}  // extern "C"
