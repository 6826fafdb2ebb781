// d2d_true_peak.hip -- true-peak cells on the device (include/dsd2dxd_amd.h, "Loudness where the PCM is"):
// d2d_true_peak_measure_device.  The definition and its arithmetic are true_peak.h, the source the host twin (d2d_loud_host.cpp) compiles
// too; the checks and the counts are d2d_loud_internal.h, also shared.
//
// The oversampling filter is a FIR: an output depends on twelve input frames and on nothing else, and every product and (for integer
// input) every sum is exact, so the frames may be spread over lanes in any way.  ONE WORKGROUP OF FOUR WAVES PER (file, row), one
// launch for all files of a call (up to MAXF; their descriptors ride in the kernel arguments).  The workgroup walks its sub-block in
// TILES of slots * RUN frames, slots = 256 / channels:
//   * STAGE: the tile's frames and the eleven in front of them go to LDS as they lie in memory, by aligned 16-byte loads, one per lane
//     and round; the frame stride (2 .. 32 bytes) need not divide 16 and a tile's edge may fall inside a 16-byte word, so the stage
//     begins at the aligned word that holds the first byte wanted.  Only the last 1 .. 15 bytes of a file, where a 16-byte load would
//     reach behind the declared frames, are read singly.
//   * FILTER: a lane is (slot, channel), channel fastest: it owns RUN consecutive frames of ONE channel, so that neighbouring lanes
//     read neighbouring samples of LDS, its window of 11 + RUN samples lives in registers, and it keeps one running maximum whatever
//     the channel count (channels that ride in the kernel arguments could not index registers).  4 x 12 v_fma_f64 per frame.  With 3 or
//     6 channels the last 256 % channels lanes stage and wait only.
// At the end the maxima meet in LDS, a tree over the slots of each channel, and the lanes of slot 0 write their channel's double with a
// plain store.  No atomics, no workgroup waits for another; every loop is bounded by counts the host computed; no scratch.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "d2d_loud_internal.h"

using namespace d2dloud;
using d2dflac::hip_fail;

namespace {

constexpr uint32_t WG = 256;
constexpr uint32_t MAXF = 64;                                      // files of one launch: 56 bytes of kernel arguments each
constexpr uint32_t RUN = 8;                                        // consecutive frames of a lane in one tile
constexpr uint32_t HIST = d2dtp::HISTORY;
constexpr uint32_t WINDOW = HIST + RUN;                            // samples a lane holds
// bytes of a stage at most: slots * channels <= 256 samples a frame-run, RUN of them, of 4 bytes; eleven frames of 32 bytes in front;
// up to 15 bytes before the first wanted one and up to 15 behind the last
constexpr uint32_t STAGE = WG * RUN * 4 + HIST * 32 + 32;
static_assert(STAGE % 16 == 0, "whole 16-byte words");

struct PeakFile {
    const uint8_t* pcm;
    double* peaks;
    uint64_t bytes;                                                // the declared frames, in bytes
    uint64_t first_frame, first_subblock;
    uint64_t end;                                                  // first_frame + frames
    uint32_t rows;                                                 // rows this file writes, > 0
    uint32_t block0;                                               // its first workgroup
};
struct PeakArgs {
    uint32_t channels, S, n_files, slots;                          // slots = 256 / channels
    PeakFile f[MAXF];
};
static_assert(sizeof(PeakFile) == 56 && sizeof(PeakArgs) <= 4096, "the descriptors ride in the kernel arguments");

// 16 bytes at the 16-byte aligned offset a of the file; the file's last 1 .. 15 bytes singly (0 behind them), nothing behind the file
__device__ __forceinline__ uint4 load16(const uint8_t* pcm, uint64_t a, uint64_t bytes) {
    if (a + 16 <= bytes) return *reinterpret_cast<const uint4*>(pcm + a);
    uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
    for (uint32_t i = 0; i < 16; ++i)
        if (a + i < bytes) w[i >> 2] |= (uint32_t)pcm[a + i] << (8 * (i & 3));
    return make_uint4(w[0], w[1], w[2], w[3]);
}

// LDS is written as 16-byte words and read as 1-, 2- or 4-byte pieces: types that may alias, so that no read moves in front of the write
typedef uint16_t __attribute__((may_alias)) lds_u16;
typedef uint32_t __attribute__((may_alias)) lds_u32;
typedef uint4 __attribute__((may_alias)) lds_u128;

// the SB little-endian bytes at byte q of the stage, in the low bits.  A 2-byte sample lies at an even q and a 4-byte one at a multiple
// of 4 (the stage begins at a multiple of 16 of the file, the frame stride is a multiple of the sample size): aligned reads.
template <uint32_t SB>
__device__ __forceinline__ uint32_t stage_sample(const uint8_t* s, uint32_t q) {
    if (SB == 2) return *reinterpret_cast<const lds_u16*>(s + q);
    if (SB == 4) return *reinterpret_cast<const lds_u32*>(s + q);
    return (uint32_t)s[q] | ((uint32_t)s[q + 1] << 8) | ((uint32_t)s[q + 2] << 16);
}

template <uint32_t SB, uint32_t DEPTH>
__global__ __launch_bounds__(WG) void true_peak_kernel(const PeakArgs a) {
    __shared__ __attribute__((aligned(16))) uint8_t s_pcm[STAGE];
    __shared__ double s_max[WG];
    // this workgroup's file and row (uniform)
    uint32_t fi = 0;
    while (fi + 1 < a.n_files && blockIdx.x >= a.f[fi + 1].block0) ++fi;
    const PeakFile fd = a.f[fi];
    const uint32_t row = blockIdx.x - fd.block0;                   // (< fd.rows: the grid is the sum of the rows)
    const uint32_t tid = threadIdx.x, ch = a.channels, slots = a.slots;
    const uint32_t slot = tid / ch, c = tid - slot * ch;
    const bool active = slot < slots;
    const uint32_t fb = ch * SB;
    const uint64_t at = (fd.first_subblock + row) * (uint64_t)a.S;
    const uint64_t to = at + a.S < fd.end ? at + a.S : fd.end;      // (the host checked: at - 11 >= first_frame or at < 11, to <= end, at < to)
    const uint32_t tile = slots * RUN;                             // frames of a tile
    double m = 0.0;
    for (uint64_t t0 = at; t0 < to; t0 += tile) {
        const uint32_t n = (uint32_t)std::min<uint64_t>(tile, to - t0);        // outputs of this tile
        const uint32_t lead = (uint32_t)std::min<uint64_t>(HIST, t0);          // frames in front of t0 the stream has: 11, or 0 at its start
        const uint64_t b0 = (t0 - lead - fd.first_frame) * fb, b1 = (t0 + n - fd.first_frame) * fb;       // the bytes wanted: <= fd.bytes
        const uint64_t a0 = b0 & ~(uint64_t)15;
        const uint32_t words = (uint32_t)((b1 - a0 + 15) >> 4);    // <= STAGE / 16
        for (uint32_t i = tid; i < words; i += WG) reinterpret_cast<lds_u128*>(s_pcm)[i] = load16(fd.pcm, a0 + 16 * (uint64_t)i, fd.bytes);
        __syncthreads();
        if (active && slot * RUN < n) {
            // window sample i is frame t0 + slot RUN - 11 + i, the stage's frame d = i + slot RUN + lead - 11: zero in front of the
            // stream (d < 0) and unused from the tile's end on
            const int32_t d0 = (int32_t)(slot * RUN + lead) - (int32_t)HIST;
            const uint32_t q0 = (uint32_t)(b0 - a0) + c * SB;
            double w[WINDOW];
#pragma unroll
            for (uint32_t i = 0; i < WINDOW; ++i) {
                const int32_t d = d0 + (int32_t)i;
                w[i] = (d >= 0 && (uint32_t)d < lead + n) ? sample(stage_sample<SB>(s_pcm, q0 + (uint32_t)d * fb), DEPTH) : 0.0;
            }
#pragma unroll
            for (uint32_t r = 0; r < RUN; ++r) {
                if (slot * RUN + r < n) {
                    const double y = d2dtp::frame_peak(&w[HIST + r]);
                    if (y > m) m = y;
                }
            }
        }
        __syncthreads();                                           // the stage is free for the next tile
    }
    // the largest of each channel: a tree over the slots
    s_max[tid] = m;
    uint32_t half = 1;
    while (half < slots) half <<= 1;
    for (half >>= 1; half; half >>= 1) {
        __syncthreads();
        if (active && slot < half && slot + half < slots) {
            const double o = s_max[tid + half * ch];
            if (o > s_max[tid]) s_max[tid] = o;
        }
    }
    if (tid < ch) fd.peaks[(uint64_t)row * ch + tid] = s_max[tid] * d2dtp::SCALE;       // (slot 0 wrote s_max[tid] last itself)
}

}  // namespace

extern "C" int d2d_true_peak_measure_device(uint32_t channels, uint32_t bit_depth, uint32_t rate, d2d_tpeak_io* io, uint32_t n_files, void* hip_stream) {
    // every check comes before the first device call and before the first count is written
    const int rc = check_call(channels, bit_depth, rate);
    if (rc != D2D_OK) return rc;
    if (n_files == 0) return D2D_OK;
    if (!io) return fail(D2D_ERR_PARAM, "no files");
    for (uint32_t f = 0; f < n_files; ++f) {
        if (io[f].frames == 0) continue;
        Plan p;
        const int prc = plan_tpeak_file(io[f], channels, rate, 16, 8, p);
        if (prc != D2D_OK) return prc;
    }
    const uint32_t sb = sample_bytes(bit_depth);
    PeakArgs a{};
    a.channels = channels; a.S = rate / 10; a.slots = WG / channels;
    uint64_t blocks = 0;
    auto launch = [&]() -> int {
        if (!a.n_files) return D2D_OK;
        const dim3 grid((uint32_t)blocks), wg(WG);
        if (sb == 2) hipLaunchKernelGGL((true_peak_kernel<2, 16>), grid, wg, 0, (hipStream_t)hip_stream, a);
        else if (sb == 3) hipLaunchKernelGGL((true_peak_kernel<3, 24>), grid, wg, 0, (hipStream_t)hip_stream, a);
        else hipLaunchKernelGGL((true_peak_kernel<4, 32>), grid, wg, 0, (hipStream_t)hip_stream, a);
        const hipError_t e = hipGetLastError();
        a.n_files = 0; blocks = 0;
        return e == hipSuccess ? D2D_OK : hip_fail(e, "true_peak_kernel");
    };
    for (uint32_t f = 0; f < n_files; ++f) {
        if (io[f].frames == 0) continue;                           // left alone
        Plan p;
        (void)plan_tpeak_file(io[f], channels, rate, 16, 8, p);
        write_tpeak_counts(io[f], p, channels);
        const uint64_t rows = p.rows();
        if (!rows) continue;
        if (a.n_files == MAXF || blocks + rows > 0x7FFFFFFFull) {
            const int lrc = launch();
            if (lrc != D2D_OK) return lrc;
        }
        PeakFile& d = a.f[a.n_files++];
        d.pcm = (const uint8_t*)io[f].pcm; d.peaks = io[f].peaks; d.bytes = (uint64_t)io[f].frames * channels * sb;
        d.first_frame = io[f].first_frame; d.first_subblock = io[f].first_subblock; d.end = io[f].first_frame + io[f].frames;
        d.rows = (uint32_t)rows; d.block0 = (uint32_t)blocks;
        blocks += rows;
    }
    return launch();
}
