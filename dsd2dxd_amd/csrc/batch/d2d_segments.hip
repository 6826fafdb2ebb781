// d2d_segments.hip -- a chunk's bookkeeping in one launch (include/dsd2dxd_amd.h): d2d_segments_move_device and
// d2d_segments_pack_device.  The checks are d2d_segments_internal.h, which the host twins (d2d_segments_host.cpp) compile too.
//
// ONE COPY ROUTINE, copy_tile, serves both calls.  A segment is cut along its DESTINATION into aligned 16-byte units, a TILE of them
// (NT * ITER units, 16 KiB) per workgroup, one unit per lane and step, so every store of the body is one aligned 16-byte store and a
// wave's stores of a step cover 1 KiB without a gap.  The source of a unit lies m = (src - dst) mod 16 bytes into an aligned 16-byte
// word -- the same m for every unit of a segment, wave-uniform -- so a lane reads the two aligned words that hold its sixteen bytes and
// shifts neighbouring dwords together with the byte-align instruction (m = 0: one word, no shift).  The second word holds the unit's
// last source byte, so both loads touch only 16-byte words that hold a byte of the declared range: they cannot leave its pages.  Only
// the first and the last unit of a segment can be partial; the lane that owns one copies its 1 .. 15 bytes singly.  Neighbouring
// lanes read the same source word twice: loads are the cheap side here, stores the scarce one.
//
// The descriptors ride in the kernel arguments with each segment's first workgroup; a workgroup finds its segment by bisection.  No
// LDS in the copy kernels, no atomics, no barrier but the table kernel's, no workgroup waits for another; every loop is bounded by a
// count from the arguments or, in the pack, by a length the table kernel has checked against its host-declared maximum.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "d2d_segments_internal.h"

using namespace d2dseg;
using d2dflac::hip_fail;

namespace {

constexpr uint32_t NT = 256;                                       // lanes of a copy workgroup
constexpr uint32_t ITER = 4;                                       // units per lane
constexpr uint64_t TILE = (uint64_t)NT * ITER * 16;                // destination bytes per workgroup
constexpr uint32_t MAXS = 96;                                      // segments of one move launch: 32 bytes of kernel arguments each
constexpr uint32_t MAXP = 128;                                     // sources of one pack launch: 16 bytes each in the copy kernel, 16 in the table kernel
constexpr uint32_t TT = 256;                                       // lanes of the table kernel: MAXP + 1 entries at most
constexpr uint64_t MAX_GRID = 0x7FFFFFFFull;

struct MoveSeg {
    uint8_t* dst;
    const uint8_t* src;
    uint64_t bytes;                                                // > 0
    uint32_t block0, reserved;                                     // its first workgroup
};
struct MoveArgs {
    uint32_t n, reserved[3];
    MoveSeg s[MAXS];
};
struct PackSrc {
    const uint8_t* base;
    uint32_t block0, reserved;
};
struct PackArgs {
    uint8_t* dst;
    const uint64_t* offsets;                                       // the entry of this launch's first source
    uint32_t n, reserved[3];
    PackSrc s[MAXP];
};
struct TableSrc {
    const uint64_t* bytes;
    uint64_t max_bytes;
};
struct TableArgs {
    uint64_t* offsets;                                             // the entry of this launch's first source
    uint32_t n, inherits;                                          // inherits: an earlier launch of the call wrote offsets[0]
    TableSrc s[MAXP];
};
static_assert(sizeof(MoveSeg) == 32 && sizeof(MoveArgs) <= 4096 && sizeof(PackArgs) <= 4096 && sizeof(TableArgs) <= 4096,
              "the descriptors ride in the kernel arguments");

// workgroups that copy `bytes` bytes to a destination whose address is `lead` mod 16
inline uint64_t tiles(uint64_t lead, uint64_t bytes) { return bytes ? (lead + bytes + TILE - 1) / TILE : 0; }

// dwords q .. q + 4 of the eight in (lo, hi), shifted down by sh bytes: the sixteen bytes from byte 4 q + sh on.  q is resolved
// at compile time in each case, so the words stay in registers.
__device__ __forceinline__ uint4 shifted(const uint4 lo, const uint4 hi, const uint32_t q, const uint32_t sh) {
    auto ab = [sh](uint32_t high, uint32_t low) { return __builtin_amdgcn_alignbyte(high, low, sh); };
    switch (q) {
    case 0: return make_uint4(ab(lo.y, lo.x), ab(lo.z, lo.y), ab(lo.w, lo.z), ab(hi.x, lo.w));
    case 1: return make_uint4(ab(lo.z, lo.y), ab(lo.w, lo.z), ab(hi.x, lo.w), ab(hi.y, hi.x));
    case 2: return make_uint4(ab(lo.w, lo.z), ab(hi.x, lo.w), ab(hi.y, hi.x), ab(hi.z, hi.y));
    default: return make_uint4(ab(hi.x, lo.w), ab(hi.y, hi.x), ab(hi.z, hi.y), ab(hi.w, hi.z));
    }
}

// tile t of the copy of n > 0 bytes from src to dst (the ranges do not overlap)
__device__ __forceinline__ void copy_tile(uint8_t* __restrict__ dst, const uint8_t* __restrict__ src, const uint64_t n, const uint64_t t) {
    const uint64_t lead = (uintptr_t)dst & 15, span = lead + n;    // the segment is bytes [lead, span) behind d0
    uint8_t* const d0 = dst - lead;
    const uint32_t m = (uint32_t)(((uintptr_t)src - (uintptr_t)dst) & 15);
#pragma unroll
    for (uint32_t k = 0; k < ITER; ++k) {
        const uint64_t b = (t * (NT * ITER) + (uint64_t)k * NT + threadIdx.x) * 16;       // this lane's unit: bytes [b, b + 16) behind d0
        if (b >= span) continue;
        if (b >= lead && b + 16 <= span) {
            const uint8_t* word = src + (b - lead) - m;            // 16-byte aligned: src + (b - lead) is m mod 16
            uint4 v = *reinterpret_cast<const uint4*>(word);
            if (m) v = shifted(v, *reinterpret_cast<const uint4*>(word + 16), m >> 2, m & 3);
            *reinterpret_cast<uint4*>(d0 + b) = v;
        } else {
            const uint64_t from = b > lead ? b : lead, to = b + 16 < span ? b + 16 : span;
            for (uint64_t j = from; j < to; ++j) d0[j] = src[j - lead];
        }
    }
}

// the last i in [0, n) with block0(i) <= block (block0(0) = 0)
template <class F>
__device__ __forceinline__ uint32_t owner(uint32_t n, uint32_t block, F block0) {
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (block0(mid) <= block) lo = mid; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(NT) void segments_move_kernel(const MoveArgs a) {
    const uint32_t i = owner(a.n, blockIdx.x, [&](uint32_t k) { return a.s[k].block0; });
    const MoveSeg s = a.s[i];
    copy_tile(s.dst, s.src, s.bytes, blockIdx.x - s.block0);
}

// the table of one launch's sources: lane k reads *bytes_k, lane k <= n writes entry k.  A length above its maximum, or a table an
// earlier launch of the call has already given up, gives UINT64_MAX in every entry of this launch, the last included, which is how a
// later launch and the copy kernels learn of it.
__global__ __launch_bounds__(TT) void segments_table_kernel(const TableArgs a) {
    __shared__ uint64_t s_len[MAXP];
    const uint32_t k = threadIdx.x;
    uint64_t len = 0;
    int bad = 0;
    if (k < a.n) { len = *a.s[k].bytes; bad = len > a.s[k].max_bytes; s_len[k] = len; }
    uint64_t first = 0;
    if (a.inherits) { first = a.offsets[0]; bad |= first == UINT64_MAX; }
    bad = __syncthreads_or(bad);
    if (k > a.n) return;
    uint64_t off = first;
    for (uint32_t i = 0; i < k; ++i) off += s_len[i];
    a.offsets[k] = bad ? UINT64_MAX : off;
}

// a call that was cut: the last entry says whether any launch gave up; then every entry says so
__global__ __launch_bounds__(TT) void segments_table_spread_kernel(uint64_t* offsets, uint32_t n) {
    if (offsets[n] != UINT64_MAX) return;
    for (uint32_t k = blockIdx.x * TT + threadIdx.x; k < n; k += gridDim.x * TT) offsets[k] = UINT64_MAX;
}

__global__ __launch_bounds__(NT) void segments_pack_kernel(const PackArgs a) {
    const uint32_t i = owner(a.n, blockIdx.x, [&](uint32_t k) { return a.s[k].block0; });
    const uint64_t at = a.offsets[i], end = a.offsets[i + 1];
    if (end == UINT64_MAX || end == at) return;                    // the table was given up (all of it), or nothing to copy
    copy_tile(a.dst + at, a.s[i].base, end - at, blockIdx.x - a.s[i].block0);      // (a tile behind the real length finds no unit)
}

}  // namespace

extern "C" int d2d_segments_move_device(const d2d_segment* seg, uint32_t n, void* hip_stream) {
    // every check comes before the first launch
    const int rc = check_move(seg, n);
    if (rc != D2D_OK) return rc;
    for (uint32_t i = 0; i < n; ++i)
        if (tiles((uintptr_t)seg[i].dst & 15, seg[i].bytes) > MAX_GRID) return fail(D2D_ERR_PARAM, "segment " + std::to_string(i) + ": longer than one launch copies");
    MoveArgs a{};
    uint64_t blocks = 0;
    auto launch = [&]() -> int {
        if (!a.n) return D2D_OK;
        hipLaunchKernelGGL(segments_move_kernel, dim3((uint32_t)blocks), dim3(NT), 0, (hipStream_t)hip_stream, a);
        const hipError_t e = hipGetLastError();
        a.n = 0; blocks = 0;
        return e == hipSuccess ? D2D_OK : hip_fail(e, "segments_move_kernel");
    };
    for (uint32_t i = 0; i < n; ++i) {
        if (seg[i].bytes == 0) continue;
        const uint64_t nb = tiles((uintptr_t)seg[i].dst & 15, seg[i].bytes);
        if (a.n == MAXS || blocks + nb > MAX_GRID) {
            const int lrc = launch();
            if (lrc != D2D_OK) return lrc;
        }
        MoveSeg& s = a.s[a.n++];
        s.dst = (uint8_t*)seg[i].dst; s.src = (const uint8_t*)seg[i].src; s.bytes = seg[i].bytes; s.block0 = (uint32_t)blocks;
        blocks += nb;
    }
    return launch();
}

extern "C" int d2d_segments_pack_device(const d2d_pack_src* src, uint32_t n, void* dst, size_t dst_capacity, uint64_t* offsets, void* hip_stream) {
    const int rc = check_pack(src, n, dst, dst_capacity, offsets, 8);
    if (rc != D2D_OK) return rc;
    for (uint32_t k = 0; k < n; ++k)
        if (tiles(15, src[k].max_bytes) > MAX_GRID) return fail(D2D_ERR_PARAM, "source " + std::to_string(k) + ": longer than one launch copies");
    hipStream_t s = (hipStream_t)hip_stream;
    // the table first, whole: a copy kernel must know that no launch gave up
    for (uint32_t k0 = 0; k0 == 0 || k0 < n; k0 += MAXP) {
        TableArgs t{};
        t.offsets = offsets + k0; t.n = std::min<uint32_t>(MAXP, n - k0); t.inherits = k0 != 0;
        for (uint32_t i = 0; i < t.n; ++i) { t.s[i].bytes = src[k0 + i].bytes; t.s[i].max_bytes = src[k0 + i].max_bytes; }
        hipLaunchKernelGGL(segments_table_kernel, dim3(1), dim3(TT), 0, s, t);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return hip_fail(e, "segments_table_kernel");
    }
    if (n > MAXP) {
        hipLaunchKernelGGL(segments_table_spread_kernel, dim3(std::min<uint32_t>((n + TT - 1) / TT, 1024)), dim3(TT), 0, s, offsets, n);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return hip_fail(e, "segments_table_spread_kernel");
    }
    PackArgs a{};
    a.dst = (uint8_t*)dst;
    uint64_t blocks = 0;
    auto launch = [&]() -> int {
        if (!a.n || !blocks) { a.n = 0; blocks = 0; return D2D_OK; }
        hipLaunchKernelGGL(segments_pack_kernel, dim3((uint32_t)blocks), dim3(NT), 0, s, a);
        const hipError_t e = hipGetLastError();
        a.n = 0; blocks = 0;
        return e == hipSuccess ? D2D_OK : hip_fail(e, "segments_pack_kernel");
    };
    for (uint32_t k = 0; k < n; ++k) {
        const uint64_t nb = tiles(15, src[k].max_bytes);           // (the destination's alignment is only known on the device)
        if (a.n == MAXP || blocks + nb > MAX_GRID) {
            const int lrc = launch();
            if (lrc != D2D_OK) return lrc;
        }
        if (a.n == 0) a.offsets = offsets + k;
        PackSrc& p = a.s[a.n++];
        p.base = (const uint8_t*)src[k].base; p.block0 = (uint32_t)blocks;
        blocks += nb;
    }
    return launch();
}
