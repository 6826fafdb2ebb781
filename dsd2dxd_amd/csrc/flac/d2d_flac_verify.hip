// d2d_flac_verify.hip -- d2d_flac_verify_device (gfx950): the frames an encode call packed into `out` are parsed, decoded and compared
// with the PCM they were made from.  The parser, its rules and the order of its checks are flac_parse.h, the host's copy
// (d2d_flac_host.cpp: d2d_flac_verify_host gives the same record for the same bytes; tests/test_gpu_flac_verify.py compares them).
//   flac_verify_status_kernel   one LANE per (file, block), FPW = 8 blocks of a file per workgroup of one wave.  A frame's bitstream is
//                               serial -- every code starts where the one before it ends -- but the frames are many and independent.
//                               A lane's time is a chain of load latencies (the next word of the frame, the PCM sample to compare), so
//                               what pays is waves in flight, not lanes per wave: with all 64 lanes on frames the bench batch is 336
//                               waves per launch on 1024 SIMDs, with 8 it is 2592 (measured: profiles/flac_verify_check.md).  The
//                               workgroup sums the sizes in front of its blocks (as flac_pack_kernel does), a scan over the wave gives
//                               each lane its frame's offset in `out`, and the lane runs verify_frame: rule 1 on the size, the header
//                               and both CRCs (the CRC-16 serially, from a table in LDS), the subframes against the PCM.  Frames
//                               start at any byte of `out`: the bit reader loads bytes up to the first 4-byte boundary and aligned
//                               words from there.  The history ring and the coefficients of an LPC subframe are 64 words per lane in
//                               LDS (word k of lane l at [k * FPW + l]: no run-time index reaches a register array, so no scratch); fixed
//                               orders keep four samples in registers.  The lane's status word -- the reason, or n << 8 -- goes to the
//                               first word of the block's workspace slot, which the pack kernel has emptied.
//   flac_verify_reduce_kernel   one workgroup per file turns the status words into the d2d_flac_check record, with plain stores.
// The two run one after the other on the caller's stream, sixteen files per pair of launches, their descriptors in the kernel
// arguments.  No atomics, no workgroup waits on another.  Every loop of the parser is bounded by n, the order or the bits of the
// frame, and every read lies in pcm[0, frames_consumed * frame_bytes), out[0, bytes_out), the size table or the result record.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "d2d_flac_internal.h"
#include "flac_parse.h"

using namespace d2dflac;

namespace {

constexpr int MAXF = 16;          // files per launch
constexpr int VT = 64;            // threads of a status workgroup: one wave
constexpr int FPW = 8;            // of which this many take a frame each; all of them sum the sizes and build the CRC table
constexpr int RT = 256;           // threads of a reduce workgroup

struct VerifyFile {
    const uint8_t* pcm;
    const uint8_t* out;
    const d2d_flac_result* result;
    const uint32_t* sizes;        // workspace: one size per block, as the encode call left them
    uint8_t* slots;               // workspace: one slot per block; its first word becomes the block's status
    d2d_flac_check* check;
    uint32_t blocks, first_block, last_n, pad;
};
struct VerifyArgs {
    VerifyFile f[MAXF];
    uint32_t channels, depth, slot_bytes, bound;
};

__global__ __launch_bounds__(VT) void flac_verify_status_kernel(const VerifyArgs a) {
    __shared__ uint16_t s_crc_tab[256];
    __shared__ int32_t s_store[2 * d2dparse::MAX_LPC_ORDER * FPW];
    const VerifyFile& fd = a.f[blockIdx.y];
    const uint32_t b0 = blockIdx.x * FPW, lane = threadIdx.x;
    if (b0 >= fd.blocks) return;
    for (uint32_t i = lane; i < 256; i += VT) s_crc_tab[i] = (uint16_t)d2dparse::crc16_entry(i);
    unsigned long long front = 0;                                   // the bytes in front of this workgroup's blocks
    for (uint32_t i = lane; i < b0; i += VT) front += fd.sizes[i];
    for (int o = VT / 2; o; o >>= 1) front += __shfl_xor(front, o);
    const uint32_t b = b0 + lane;
    const uint32_t size = lane < FPW && b < fd.blocks ? fd.sizes[b] : 0;
    unsigned long long upto = size;                                 // inclusive scan over the wave
    for (int o = 1; o < VT; o <<= 1) { const unsigned long long t = __shfl_up(upto, o); if ((int)lane >= o) upto += t; }
    __syncthreads();
    if (lane >= FPW || b >= fd.blocks) return;
    const unsigned long long off = front + upto - size;
    const bool last = b + 1 == fd.blocks;
    const uint32_t n = last ? fd.last_n : BS;
    uint32_t reason = D2D_FLAC_BAD_SIZE;
    if (d2dparse::size_ok(off, size, fd.result->bytes_out, a.bound, last)) {
        const d2dparse::Expect ex{a.channels, a.depth, n, fd.first_block + b};
        const size_t frame_bytes = (size_t)a.channels * (a.depth == 16 ? 2 : 3);
        reason = d2dparse::verify_frame(fd.out + off, size, true, ex, fd.pcm + (size_t)b * BS * frame_bytes, s_crc_tab, s_store + lane, FPW, nullptr);
    }
    *reinterpret_cast<uint32_t*>(fd.slots + (size_t)b * a.slot_bytes) = d2dparse::status_word(reason, n);
}

__global__ __launch_bounds__(RT) void flac_verify_reduce_kernel(const VerifyArgs a) {
    __shared__ unsigned long long s_samples[RT / 64];
    __shared__ uint32_t s_bad[RT / 64], s_first[RT / 64];
    const VerifyFile& fd = a.f[blockIdx.x];
    const uint32_t tid = threadIdx.x;
    auto status = [&](uint32_t b) { return *reinterpret_cast<const uint32_t*>(fd.slots + (size_t)b * a.slot_bytes); };
    unsigned long long samples = 0;
    uint32_t bad = 0, first = 0xFFFFFFFFu;
    for (uint32_t b = tid; b < fd.blocks; b += RT) {
        const uint32_t w = status(b);
        if (w & 0xFFu) { ++bad; first = min(first, b); }
        else samples += w >> 8;
    }
    for (int o = 32; o; o >>= 1) {
        samples += __shfl_xor(samples, o); bad += __shfl_xor(bad, o); first = min(first, (uint32_t)__shfl_xor(first, o));
    }
    if ((tid & 63) == 0) { s_samples[tid >> 6] = samples; s_bad[tid >> 6] = bad; s_first[tid >> 6] = first; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < RT / 64; ++w) { samples += s_samples[w]; bad += s_bad[w]; first = min(first, s_first[w]); }
        d2d_flac_check c;
        c.samples_checked = samples; c.blocks_checked = fd.blocks; c.bad_blocks = bad; c.first_bad_block = first;
        c.first_bad_reason = bad ? status(first) & 0xFFu : (uint32_t)D2D_FLAC_BAD_NONE;
        *fd.check = c;
    }
}

}  // namespace

extern "C" int d2d_flac_verify_device(uint32_t channels, uint32_t bit_depth, const d2d_flac_io* io, uint32_t n_files,
                                      void* workspace, size_t workspace_bytes, d2d_flac_check* checks, void* hip_stream) {
    // every check comes before the first device call
    if (!depth_ok(bit_depth)) return fail(D2D_ERR_PARAM, "FLAC holds 16, 20 or 24-bit integers (Invalid bit depth)");
    if (channels == 0 || channels > 8) return fail(D2D_ERR_PARAM, "FLAC holds 1 to 8 channels (Invalid channel count)");
    if (!io || n_files == 0) return fail(D2D_ERR_PARAM, "no files");
    if (!checks || ((uintptr_t)checks & 7)) return fail(D2D_ERR_PARAM, "checks must be an 8-byte aligned pointer the GPU can address");
    size_t need = 0, any_blocks = 0;
    for (uint32_t f = 0; f < n_files; ++f) {
        const d2d_flac_io& x = io[f];
        const size_t blocks = block_count(x.frames, x.final);
        if ((uint64_t)x.first_block + blocks > (1ull << 31)) return fail(D2D_ERR_PARAM, "frame numbers are 31 bits: first_block + blocks exceeds 2^31");
        if (!x.result) return fail(D2D_ERR_PARAM, "null result record");
        if (((uintptr_t)x.pcm & 15) || ((uintptr_t)x.out & 15)) return fail(D2D_ERR_PARAM, "pcm and out device pointers must be 16-byte aligned");
        if (blocks && (!x.pcm || !x.out)) return fail(D2D_ERR_PARAM, "pcm and out device pointers must be non-null");
        need += d2d_flac_workspace_bytes(channels, bit_depth, x.frames, x.final);
        any_blocks += blocks;
    }
    if (any_blocks && (!workspace || ((uintptr_t)workspace & 15))) return fail(D2D_ERR_PARAM, "workspace must be a 16-byte aligned device pointer");
    if (workspace_bytes < need) return fail(D2D_ERR_CAPACITY, "workspace below the sum of d2d_flac_workspace_bytes");

    hipStream_t s = (hipStream_t)hip_stream;
    uint8_t* ws = (uint8_t*)workspace;
    for (uint32_t f0 = 0; f0 < n_files; f0 += MAXF) {
        const uint32_t nf = std::min<uint32_t>(MAXF, n_files - f0);
        VerifyArgs a{};
        a.channels = channels; a.depth = bit_depth; a.slot_bytes = (uint32_t)slot_bytes(channels, bit_depth); a.bound = (uint32_t)frame_bound(channels, bit_depth, BS);
        uint32_t max_blocks = 0;
        for (uint32_t i = 0; i < nf; ++i) {                         // the workspace is walked as the encode call walked it
            const d2d_flac_io& x = io[f0 + i];
            const size_t blocks = block_count(x.frames, x.final);
            VerifyFile& d = a.f[i];
            d.pcm = (const uint8_t*)x.pcm; d.out = (const uint8_t*)x.out; d.result = x.result; d.check = checks + f0 + i;
            d.sizes = (const uint32_t*)ws; d.slots = ws + align16(4 * blocks);
            d.blocks = (uint32_t)blocks; d.first_block = x.first_block;
            d.last_n = (x.final && x.frames % BS) ? (uint32_t)(x.frames % BS) : BS;
            ws += d2d_flac_workspace_bytes(channels, bit_depth, x.frames, x.final);
            max_blocks = std::max(max_blocks, d.blocks);
        }
        if (max_blocks) {
            hipLaunchKernelGGL(flac_verify_status_kernel, dim3((max_blocks + FPW - 1) / FPW, nf), dim3(VT), 0, s, a);
            const hipError_t e = hipGetLastError();
            if (e != hipSuccess) return hip_fail(e, "flac_verify_status_kernel");
        }
        hipLaunchKernelGGL(flac_verify_reduce_kernel, dim3(nf), dim3(RT), 0, s, a);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return hip_fail(e, "flac_verify_reduce_kernel");
    }
    return D2D_OK;
}
