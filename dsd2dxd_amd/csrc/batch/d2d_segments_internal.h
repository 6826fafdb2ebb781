// d2d_segments_internal.h -- what the device calls (d2d_segments.hip) and their host twins (d2d_segments_host.cpp) share: the checks
// of include/dsd2dxd_amd.h, "A chunk's bookkeeping in one launch".  Host code only.
#pragma once
#include <algorithm>
#include <vector>

#include "../flac/d2d_flac_internal.h"

namespace d2dseg {

using d2dflac::fail;

// the checks of a move call: no null pointer, no range that wraps, and no dst range that overlaps a src or another dst range.  Ranges
// of 0 bytes do not take part.  One sweep over the ranges sorted by their first byte: a range overlaps an earlier one exactly when it
// begins below that one's end, so the largest end so far of all ranges, and of the dst ranges alone, decide.
inline int check_move(const d2d_segment* seg, uint32_t n) {
    if (n == 0) return D2D_OK;
    if (!seg) return fail(D2D_ERR_PARAM, "no segments");
    struct Range { uintptr_t at, end; bool dst; };
    std::vector<Range> r;
    r.reserve(2 * (size_t)n);
    for (uint32_t i = 0; i < n; ++i) {
        if (seg[i].bytes == 0) continue;
        const uintptr_t d = (uintptr_t)seg[i].dst, s = (uintptr_t)seg[i].src;
        if (!d || !s) return fail(D2D_ERR_PARAM, "segment " + std::to_string(i) + ": null pointer");
        if (d + seg[i].bytes < d || s + seg[i].bytes < s) return fail(D2D_ERR_PARAM, "segment " + std::to_string(i) + ": the range wraps the address space");
        r.push_back(Range{d, d + seg[i].bytes, true});
        r.push_back(Range{s, s + seg[i].bytes, false});
    }
    std::sort(r.begin(), r.end(), [](const Range& a, const Range& b) { return a.at < b.at; });
    uintptr_t end_all = 0, end_dst = 0;
    for (const Range& x : r) {
        if (x.at < (x.dst ? end_all : end_dst)) return fail(D2D_ERR_PARAM, "a dst range overlaps another range of the call");
        end_all = std::max(end_all, x.end);
        if (x.dst) end_dst = std::max(end_dst, x.end);
    }
    return D2D_OK;
}

// the checks of a pack call; align: what `offsets` must have (8 on the device; the twin reads and writes it bytewise: 1)
inline int check_pack(const d2d_pack_src* src, uint32_t n, const void* dst, size_t dst_capacity, const uint64_t* offsets, uintptr_t align) {
    if (!offsets || ((uintptr_t)offsets & (align - 1))) return fail(D2D_ERR_PARAM, "offsets must be a non-null, 8-byte aligned pointer");
    if (n && !src) return fail(D2D_ERR_PARAM, "no sources");
    size_t sum = 0;
    for (uint32_t k = 0; k < n; ++k) {
        if (!src[k].bytes) return fail(D2D_ERR_PARAM, "source " + std::to_string(k) + ": null length pointer");
        if ((uintptr_t)src[k].bytes & (align - 1)) return fail(D2D_ERR_PARAM, "source " + std::to_string(k) + ": the length pointer must be 8-byte aligned");
        if (src[k].max_bytes && !src[k].base) return fail(D2D_ERR_PARAM, "source " + std::to_string(k) + ": null base");
        if (sum + src[k].max_bytes < sum) return fail(D2D_ERR_CAPACITY, "the sum of max_bytes exceeds dst_capacity");
        sum += src[k].max_bytes;
    }
    if (sum > dst_capacity) return fail(D2D_ERR_CAPACITY, "the sum of max_bytes exceeds dst_capacity");
    if (sum && !dst) return fail(D2D_ERR_PARAM, "null dst");
    return D2D_OK;
}

}  // namespace d2dseg
