// d2d_loud.hip -- loudness cells on the device (include/dsd2dxd_amd.h, "Loudness where the PCM is"): d2d_loud_measure_device.  The
// sample conversions, the two biquads and the sums are loud_meter.h, the source the host twin (d2d_loud_host.cpp) compiles too; the
// checks and the counts are d2d_loud_internal.h, also shared.
//
// The filter of every sub-block starts from rest two sub-blocks earlier, so a (file, sub-block, channel) unit depends on no other: ONE
// LANE PER UNIT, one launch for all files of a call (up to MAXF; their descriptors ride in the kernel arguments).  A workgroup is one
// wave and belongs to one file; its lanes are 64 neighbouring units, channel fastest, so the channels of a frame share cache lines.  A
// lane walks its up to 3 S frames in order -- the walk is the serial part, 3 S steps long whatever the batch -- and writes its cell with
// one plain 16-byte store.  No atomics, no workgroup waits for another (no barrier either: a lane reads only the LDS column it wrote);
// every loop is bounded by the counts the host computed.
//
// THE FETCH.  A lane's frames are contiguous in memory, so it reads them as a stream of aligned 16-byte loads, a WINDOW of WIN bytes at a
// time, and parks the window in its own COL bytes of LDS, from where the samples come back by their byte offsets (the frame stride
// need not divide 16).  COL is an odd number of words, so the lanes' reads of one offset fall on different banks.  The window behind
// the one in work is already on its way in registers while the filter runs, which hides the memory latency: with one 4-byte load per
// sample, eight frames ahead and no LDS, the same batch took twice as long (profiles/loudness_check.md has the three forms that were
// timed).  Only the last 1 .. 15 bytes of a file, where a 16-byte load would reach behind the declared frames, are read singly.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "d2d_loud_internal.h"

using namespace d2dloud;
using d2dflac::hip_fail;

namespace {

constexpr uint32_t WAVE = 64;
constexpr uint32_t MAXF = 64;                                      // files of one launch: 56 bytes of kernel arguments each
constexpr uint32_t WIN = 128;                                      // bytes a window advances: a cache line
constexpr uint32_t NV = WIN / 16 + 1;                              // its 16-byte loads: one more than WIN, for the sample that straddles its end
constexpr uint32_t COL = 16 * NV + 4;                              // bytes of LDS per lane: the window and one word, 37 words
static_assert(COL % 4 == 0 && (COL / 4) % 2 == 1, "whole words, an odd number of them");

struct LoudFile {
    const uint8_t* pcm;
    d2d_loud_cell* cells;
    uint64_t bytes;                                                // the declared frames, in bytes
    uint64_t first_frame, first_subblock;
    uint64_t end;                                                  // first_frame + frames
    uint32_t units;                                                // cells this file writes: rows * channels, > 0
    uint32_t block0;                                               // its first workgroup
};
struct LoudArgs {
    Coef k;
    uint32_t channels, S, n_files, reserved;
    LoudFile f[MAXF];
};
static_assert(sizeof(LoudFile) == 56 && sizeof(LoudArgs) <= 4096, "the descriptors ride in the kernel arguments");
static_assert(sizeof(d2d_loud_cell) == 16, "a cell is one 16-byte store");

// 16 bytes at the 16-byte aligned offset a of the file; the file's last 1 .. 15 bytes singly (0 behind them), nothing behind the file
__device__ __forceinline__ uint4 load16(const uint8_t* pcm, uint64_t a, uint64_t bytes) {
    if (a + 16 <= bytes) return *reinterpret_cast<const uint4*>(pcm + a);
    uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
    for (uint32_t i = 0; i < 16; ++i)
        if (a + i < bytes) w[i >> 2] |= (uint32_t)pcm[a + i] << (8 * (i & 3));
    return make_uint4(w[0], w[1], w[2], w[3]);
}

// LDS is written as words and read as 1-, 2- or 4-byte pieces: types that may alias, so that no read moves in front of the write
typedef uint16_t __attribute__((may_alias)) lds_u16;
typedef uint32_t __attribute__((may_alias)) lds_u32;

// the SB little-endian bytes at byte q of the lane's window `col`, in the low bits.  A 2-byte sample lies at an even q and a 4-byte
// one at a multiple of 4 (the frame stride is a multiple of the sample size, COL of 4): aligned reads.
template <uint32_t SB>
__device__ __forceinline__ uint32_t window_sample(const uint8_t* col, uint32_t q) {
    if (SB == 2) return *reinterpret_cast<const lds_u16*>(col + q);
    if (SB == 4) return *reinterpret_cast<const lds_u32*>(col + q);
    return (uint32_t)col[q] | ((uint32_t)col[q + 1] << 8) | ((uint32_t)col[q + 2] << 16);
}

template <uint32_t SB, uint32_t DEPTH>
__global__ __launch_bounds__(WAVE) void loud_cells_kernel(const LoudArgs a) {
    __shared__ __attribute__((aligned(16))) uint8_t s_win[WAVE * COL];
    // this workgroup's file (wave-uniform)
    uint32_t fi = 0;
    while (fi + 1 < a.n_files && blockIdx.x >= a.f[fi + 1].block0) ++fi;
    const LoudFile fd = a.f[fi];
    const uint32_t lane = threadIdx.x;
    const uint32_t unit = (blockIdx.x - fd.block0) * WAVE + lane;
    if (unit >= fd.units) return;
    const uint32_t row = unit / a.channels, c = unit - row * a.channels;
    const uint64_t S = a.S, j = fd.first_subblock + row;
    const uint64_t from = start_subblock(j) * S, at = j * S, to = at + S < fd.end ? at + S : fd.end;
    const uint32_t fb = a.channels * SB;
    uint64_t o = (from - fd.first_frame) * fb + (uint64_t)c * SB;  // the next sample's byte (the host checked: from >= first_frame, to <= end)
    uint32_t quiet = (uint32_t)(at - from), counted = (uint32_t)(to - at);      // frames of the pre-roll and of the sub-block still to come: <= 2 S, 1 .. S
    const uint64_t stop = o + (uint64_t)(quiet + counted - 1) * fb + SB;        // behind this lane's last sample: <= fd.bytes
    Unit u;
    uint8_t* col = s_win + lane * COL;
    uint64_t base = o & ~(uint64_t)15;                             // the window on its way: bytes [base, base + 16 NV)
    uint32_t q = (uint32_t)(o - base);                             // the next sample's byte in it
    uint4 next[NV];
#pragma unroll
    for (uint32_t i = 0; i < NV; ++i) next[i] = load16(fd.pcm, base + 16 * i, fd.bytes);
    while (quiet + counted) {
        // the window that arrived goes to this lane's bytes of LDS, the one behind it is asked for, and the filter takes every sample
        // that begins in the first WIN bytes of the one in LDS (at least 4: a frame is at most 32 bytes)
#pragma unroll
        for (uint32_t i = 0; i < NV; ++i) {
            lds_u32* w = reinterpret_cast<lds_u32*>(col + 16 * i);
            w[0] = next[i].x; w[1] = next[i].y; w[2] = next[i].z; w[3] = next[i].w;
        }
        base += WIN;
        if (base < stop) {
#pragma unroll
            for (uint32_t i = 0; i < NV; ++i) next[i] = load16(fd.pcm, base + 16 * i, fd.bytes);
        }
        for (; q < WIN && quiet; q += fb, --quiet) preroll(u, a.k, sample(window_sample<SB>(col, q), DEPTH));
        for (; q < WIN && counted; q += fb, --counted) measure(u, a.k, sample(window_sample<SB>(col, q), DEPTH));
        q -= WIN;                                                  // (only where frames are left: then q >= WIN)
    }
    *reinterpret_cast<double2*>(fd.cells + unit) = make_double2(u.energy, u.peak);
}

}  // namespace

extern "C" int d2d_loud_measure_device(uint32_t channels, uint32_t bit_depth, uint32_t rate, d2d_loud_io* io, uint32_t n_files, void* hip_stream) {
    // every check comes before the first device call and before the first count is written
    const int rc = check_call(channels, bit_depth, rate);
    if (rc != D2D_OK) return rc;
    if (n_files == 0) return D2D_OK;
    if (!io) return fail(D2D_ERR_PARAM, "no files");
    for (uint32_t f = 0; f < n_files; ++f) {
        if (io[f].frames == 0) continue;
        Plan p;
        const int prc = plan_file(io[f], channels, rate, 16, p);
        if (prc != D2D_OK) return prc;
    }
    const uint32_t sb = sample_bytes(bit_depth);
    LoudArgs a{};
    a.k = host_coefficients(rate); a.channels = channels; a.S = rate / 10;
    uint64_t blocks = 0;
    auto launch = [&]() -> int {
        if (!a.n_files) return D2D_OK;
        const dim3 grid((uint32_t)blocks), wg(WAVE);
        if (sb == 2) hipLaunchKernelGGL((loud_cells_kernel<2, 16>), grid, wg, 0, (hipStream_t)hip_stream, a);
        else if (sb == 3) hipLaunchKernelGGL((loud_cells_kernel<3, 24>), grid, wg, 0, (hipStream_t)hip_stream, a);
        else hipLaunchKernelGGL((loud_cells_kernel<4, 32>), grid, wg, 0, (hipStream_t)hip_stream, a);
        const hipError_t e = hipGetLastError();
        a.n_files = 0; blocks = 0;
        return e == hipSuccess ? D2D_OK : hip_fail(e, "loud_cells_kernel");
    };
    for (uint32_t f = 0; f < n_files; ++f) {
        if (io[f].frames == 0) continue;                           // left alone
        Plan p;
        (void)plan_file(io[f], channels, rate, 16, p);
        write_counts(io[f], p, channels);
        const uint64_t units = p.rows() * channels;
        if (!units) continue;
        const uint64_t nb = (units + WAVE - 1) / WAVE;
        if (a.n_files == MAXF || blocks + nb > 0x7FFFFFFFull) {
            const int lrc = launch();
            if (lrc != D2D_OK) return lrc;
        }
        LoudFile& d = a.f[a.n_files++];
        d.pcm = (const uint8_t*)io[f].pcm; d.cells = io[f].cells; d.bytes = (uint64_t)io[f].frames * channels * sb;
        d.first_frame = io[f].first_frame; d.first_subblock = io[f].first_subblock; d.end = io[f].first_frame + io[f].frames;
        d.units = (uint32_t)units; d.block0 = (uint32_t)blocks;
        blocks += nb;
    }
    return launch();
}
