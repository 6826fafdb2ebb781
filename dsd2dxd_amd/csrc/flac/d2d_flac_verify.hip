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
//                               This is D2D_FLAC_VERIFY_SERIAL, and the meaning of every record.
//   flac_verify_coop_kernel     D2D_FLAC_VERIFY_COOP (and AUTO): one WORKGROUP of 1024 threads per (file, block), the encoders' shape.  The
//                               verifier holds the PCM, so nothing but a few fields is serial for it: flac_expect.h has the rule (E1
//                               to E6), why it is sound, and the small arithmetic, shared with the host twin.  Per frame:
//                                 1. the sizes in front of the block are summed over the workgroup; rule 1 on the size
//                                 2. the frame comes into LDS as big-endian words (the encoders' image): aligned words shifted into
//                                    place, the first and last bytes singly, nothing outside [frame, frame + size); the first 17
//                                    bytes also as they are, for parse_header (rules 2 to 4)
//                                 3. the CRC-16 by the encoders' tree, frame_crc16, over the image with its last two bytes cleared
//                                 4. per subframe, in order: every thread walks the head (walk_subframe on the image -- a dozen LDS
//                                    reads); the channel's samples (mid and side formed from the PCM) go to one 16 KB plane, sample
//                                    i to thread i % 1024: reads and writes without bank conflicts; verbatim and warm-up samples are
//                                    compared where they stand; every residual comes from the ORIGINAL samples in the plane, and
//                                    its zigzag value replaces the sample there; wave 0 walks the partitions -- parameter, the sum
//                                    of that partition's code lengths over its lanes (DPP), next parameter: at most 64 short steps,
//                                    never one per sample -- and leaves the parameters and the subframe's end in LDS; then thread t
//                                    takes samples 4t .. 4t+3 back, scan_starts turns lengths into positions, and every code is
//                                    compared with the bits at its position
//                                 5. padding and end
//                               A position that would pass the frame's last body bit is a reject decided before the read.  Every
//                               reject -- and rule 1 -- hands the block to one lane running verify_frame on the frame in global
//                               memory, as the serial kernel does; its answer is the status, with FALLBACK_BIT set.  The frame lives
//                               in LDS because every code is read once at a data-dependent bit position and the CRC tree reads
//                               every byte: 123 KB for eight channels at 24 bits, beside the plane 143 KB of the CU's 160.
//   flac_verify_reduce_kernel   one workgroup per file turns the status words into the d2d_flac_check record (and, where asked for, the
//                               d2d_flac_verify_stats), with plain stores.
// A status kernel and the reduce kernel run one after the other on the caller's stream, sixteen files per pair of launches, their
// descriptors in the kernel arguments.  No atomics on global memory, no workgroup waits on another.  Every loop of the parser is
// bounded by n, the order or the bits of the frame, and every read lies in pcm[0, frames_consumed * frame_bytes), out[0, bytes_out), the size table or the result record.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <mutex>

#include "d2d_flac_internal.h"
#include "flac_device.h"
#include "flac_expect.h"

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
    d2d_flac_verify_stats* stats; // or null
    uint32_t blocks, first_block, last_n, pad;
};
struct VerifyArgs {
    VerifyFile f[MAXF];
    uint32_t channels, depth, slot_bytes, bound;
    uint32_t serial, pad;         // the serial status kernel wrote the words: every block is the serial parser's
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

// ---- the cooperative verifier ----------------------------------------------------------------------------------------------------

struct LdsImage {                                                   // flac_expect.h's Img over the frame in LDS, zeros behind the frame
    const uint32_t* img;
    __device__ __forceinline__ uint32_t word(uint32_t w) const { return img[w]; }
};
struct CoopLds {                                                    // the static LDS; the image is the dynamic part
    uint32_t plane[BS];                                             // one coded signal's samples, then their zigzag residuals
    uint32_t wtot[NW][1];
    uint16_t crc_tab[256], crc[NT];
    unsigned long long front[NW];
    int32_t coef[d2dparse::MAX_LPC_ORDER];
    int32_t store[2 * d2dparse::MAX_LPC_ORDER];                     // the serial parser's ring and coefficients
    uint32_t kpart[1u << d2dexpect::MAX_PORDER];
    uint32_t chain_end, chain_bad;
    uint8_t hdr[d2dparse::MAX_HEADER + 3];
};
// the words of the image a launch allocates: the largest frame, one word for a field that ends in the last, rounded to 16 bytes
__host__ __device__ inline size_t coop_image_bytes(uint32_t bound) { return ((size_t)bound + 4 + 15) & ~(size_t)15; }

// Step 2: bytes 4w .. 4w+3 of the frame as a big-endian word.  `shift` is the frame's address modulo 4: an inner word is two aligned
// loads that lie wholly in the frame, an edge word goes byte by byte.
__device__ __forceinline__ uint32_t frame_word(const uint8_t* frame, uint32_t size, uint32_t shift, uint32_t w) {
    const uint32_t at = 4 * w;
    if (shift == 0 && at + 4 <= size) return __builtin_bswap32(*reinterpret_cast<const uint32_t*>(frame + at));
    if (shift != 0 && at >= shift && at - shift + 8 <= size) {
        const uint32_t* q = reinterpret_cast<const uint32_t*>(frame + at - shift);
        const uint64_t two = ((uint64_t)q[1] << 32) | q[0];
        return __builtin_bswap32((uint32_t)(two >> (8 * shift)));
    }
    uint32_t v = 0;
    for (uint32_t i = 0; i < 4; ++i) v = (v << 8) | (at + i < size ? (uint32_t)frame[at + i] : 0u);
    return v;
}

// E1 to E6 of flac_expect.h on the frame in `img`; the whole workgroup, every branch that holds a barrier uniform.  True: good.
__device__ __forceinline__ bool coop_accept(uint32_t* img, CoopLds& s, uint32_t size, const d2dparse::Expect& ex, const uint8_t* pcm, const Block B) {
    using namespace d2dexpect;
    const uint32_t tid = B.tid, n = ex.n;
    const LdsImage image{img};
    // E1: rules 2 to 5
    d2dparse::Header h;
    if (d2dparse::parse_header(s.hdr, size, ex, h) || size < h.bytes + 2) return false;
    const uint32_t body_end = 8 * (size - 2), stored = peek(image, body_end, 16);
    __syncthreads();
    if (tid == 0) for (uint32_t j = size - 2; j < size; ++j) img[j >> 2] &= ~(0xFFu << (24 - 8 * (j & 3)));
    __syncthreads();
    frame_crc16(img, size - 2, s.crc_tab, s.crc, tid);
    if (peek(image, body_end, 16) != stored) return false;

    const uint32_t channels = h.assignment < 8 ? h.assignment + 1 : 2;
    d2dparse::VerifySig sig{pcm, ex.channels, ex.depth, 1, nullptr};
    uint32_t pos = 8 * h.bytes;
    for (uint32_t c = 0; c < channels; ++c) {
        sig.begin(c, h.assignment);
        const uint32_t bps = ex.depth + (sig.kind == 2 ? 1 : 0);
        ImageReader<LdsImage> br(image, pos, body_end);
        SubHead sh;
        __syncthreads();                                            // (the last channel's readers of coef and the plane are through)
        if (!walk_subframe(br, n, bps, sh, s.coef)) return false;   // every thread the same fields: the same words to coef
        const uint32_t plain = sh.verbatim ? n : sh.order;
        if ((uint64_t)pos + 8 + (uint64_t)plain * bps > body_end) return false;
        bool bad = false;
#pragma unroll
        for (int j = 0; j < SPT; ++j) {                             // sample i of thread i % NT
            const uint32_t i = tid + NT * j;
            if (i >= n) continue;
            const int32_t x = coded_sample(sig, i);
            s.plane[i] = (uint32_t)x;
            if (i < plain && !sample_matches(image, pos + 8 + i * bps, x, bps)) bad = true;
        }
        if (sh.verbatim) {
            pos += 8 + n * bps;
            if (__syncthreads_or(bad)) return false;
            continue;
        }
        __syncthreads();
        uint32_t u[SPT];
#pragma unroll
        for (int j = 0; j < SPT; ++j) {
            const uint32_t i = tid + NT * j;
            u[j] = 0;
            if (i < sh.order || i >= n) continue;
            const int32_t* x = reinterpret_cast<const int32_t*>(s.plane) + i;
            const uint64_t z = zigzag((int64_t)*x - predict(sh, x, s.coef));
            if (z >> 32) bad = true;                                // E3
            u[j] = (uint32_t)z;
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < SPT; ++j) if (tid + NT * j < n) s.plane[tid + NT * j] = u[j];
        __syncthreads();
        // the partitions, one after the other, on wave 0: each lane sums the lengths of its samples of the partition; a sum beyond the
        // body is a reject and adds nothing, so that no sum leaves 32 bits (E4)
        const uint32_t psz = n >> sh.porder;
        if (B.wave == 0) {
            uint32_t p = pos + sh.bits;
            bool cbad = false;
            for (uint32_t j = 0; j < (1u << sh.porder) && !cbad; ++j) {
                if (p + 5 > body_end) { cbad = true; break; }
                const uint32_t k = peek(image, p, 5);
                if (k == 31) { cbad = true; break; }
                uint32_t mine = 0;
                bool over = false;
                for (uint32_t i = partition_first(j, psz, sh.order) + B.lane; i < (j + 1) * psz; i += 64) {
                    const uint64_t len = code_len(s.plane[i], k);
                    if (len > body_end || mine + len > body_end) over = true;
                    else mine += (uint32_t)len;
                }
                if (__ballot(over)) { cbad = true; break; }
                p += 5 + wave_sum(mine);
                if (p > body_end) cbad = true;
                if (B.lane == 0) s.kpart[j] = k;
            }
            if (B.lane == 0) { s.chain_end = p; s.chain_bad = cbad; }
        }
        __syncthreads();
        if (s.chain_bad) return false;
        // thread t's samples 4t .. 4t+3: lengths, positions, the compare.  Partition j's parameter lies in front of its codes, so a code
        // starts 5 (j + 1) bits behind the lengths in front of it.
        const uint4 mine4 = *reinterpret_cast<const uint4*>(&s.plane[B.i0]);
        const uint32_t own[SPT] = {mine4.x, mine4.y, mine4.z, mine4.w};
        uint32_t kk[SPT], len[SPT], sum[1] = {0}, start[1];
#pragma unroll
        for (int j = 0; j < SPT; ++j) {
            const uint32_t i = B.i0 + j;
            const bool coded = i >= sh.order && i < n;
            kk[j] = coded ? s.kpart[i / psz] : 0;
            len[j] = coded ? (uint32_t)code_len(own[j], kk[j]) : 0;
            sum[0] += len[j];
        }
        const uint32_t end = scan_starts<1>(start, sum, pos + sh.bits, s.wtot, B) + (5u << sh.porder);
        uint32_t at = start[0];
#pragma unroll
        for (int j = 0; j < SPT; ++j) {
            const uint32_t i = B.i0 + j;
            if (i >= sh.order && i < n) {
                const uint32_t code_at = at + 5 * (i / psz + 1);
                if (code_at + len[j] > end || !code_matches(image, code_at, own[j], kk[j])) bad = true;
            }
            at += len[j];
        }
        if (end != s.chain_end) bad = true;                         // (the two sums are of the same lengths)
        pos = end;
        if (__syncthreads_or(bad)) return false;
    }
    return tail_ok(image, pos, body_end);
}

__global__ __launch_bounds__(NT) void flac_verify_coop_kernel(const VerifyArgs a) {
    extern __shared__ __align__(16) unsigned char smem[];           // the frame image
    __shared__ CoopLds s;
    uint32_t* img = reinterpret_cast<uint32_t*>(smem);
    const VerifyFile& fd = a.f[blockIdx.y];
    const uint32_t b = blockIdx.x;
    if (b >= fd.blocks) return;
    Block B{};
    B.tid = threadIdx.x; B.lane = B.tid & 63u; B.wave = B.tid >> 6; B.i0 = B.tid * SPT;
    const uint32_t tid = B.tid;
    // step 1
    unsigned long long front = 0;                                   // the bytes in front of this block, as the host adds them: modulo 2^64
    for (uint32_t i = tid; i < b; i += NT) front += fd.sizes[i];
    for (int o = 32; o; o >>= 1) front += __shfl_xor(front, o);
    if (B.lane == 0) s.front[B.wave] = front;
    build_crc_tab(s.crc_tab, tid);
    __syncthreads();
    unsigned long long off = 0;
    for (int w = 0; w < NW; ++w) off += s.front[w];
    const uint32_t size = fd.sizes[b];
    const bool last = b + 1 == fd.blocks;
    const uint32_t n = last ? fd.last_n : BS;
    const d2dparse::Expect ex{a.channels, a.depth, n, fd.first_block + b};
    const uint8_t* pcm = fd.pcm + (size_t)b * BS * a.channels * (a.depth == 16 ? 2 : 3);
    const bool sized = d2dparse::size_ok(off, size, fd.result->bytes_out, a.bound, last);
    bool good = false;
    if (sized) {                                                    // (uniform)
        // step 2
        const uint8_t* frame = fd.out + off;
        const uint32_t shift = (uint32_t)((uintptr_t)frame & 3u), words = (uint32_t)(coop_image_bytes(a.bound) / 4);
        for (uint32_t w = tid; w < words; w += NT) img[w] = 4 * w < size ? frame_word(frame, size, shift, w) : 0u;
        if (tid < d2dparse::MAX_HEADER && tid < size) s.hdr[tid] = frame[tid];
        __syncthreads();
        good = coop_accept(img, s, size, ex, pcm, B);
    }
    if (tid != 0) return;
    uint32_t word = d2dparse::status_word(D2D_FLAC_BAD_NONE, n);
    if (!good) {
        const uint32_t reason = sized ? d2dparse::verify_frame(fd.out + off, size, true, ex, pcm, s.crc_tab, s.store, 1, nullptr) : (uint32_t)D2D_FLAC_BAD_SIZE;
        word = d2dparse::status_word(reason, n) | d2dexpect::FALLBACK_BIT;
    }
    *reinterpret_cast<uint32_t*>(fd.slots + (size_t)b * a.slot_bytes) = word;
}

__global__ __launch_bounds__(RT) void flac_verify_reduce_kernel(const VerifyArgs a) {
    __shared__ unsigned long long s_samples[RT / 64];
    __shared__ uint32_t s_bad[RT / 64], s_first[RT / 64], s_slow[RT / 64];
    const VerifyFile& fd = a.f[blockIdx.x];
    const uint32_t tid = threadIdx.x;
    auto status = [&](uint32_t b) { return *reinterpret_cast<const uint32_t*>(fd.slots + (size_t)b * a.slot_bytes); };
    unsigned long long samples = 0;
    uint32_t bad = 0, first = 0xFFFFFFFFu, slow = 0;                // slow: the blocks the serial parser decided
    for (uint32_t b = tid; b < fd.blocks; b += RT) {
        const uint32_t w = status(b);
        if (w & d2dexpect::FALLBACK_BIT) ++slow;
        if (w & 0xFFu) { ++bad; first = min(first, b); }
        else samples += (w & ~d2dexpect::FALLBACK_BIT) >> 8;
    }
    for (int o = 32; o; o >>= 1) {
        samples += __shfl_xor(samples, o); bad += __shfl_xor(bad, o); first = min(first, (uint32_t)__shfl_xor(first, o)); slow += __shfl_xor(slow, o);
    }
    if ((tid & 63) == 0) { s_samples[tid >> 6] = samples; s_bad[tid >> 6] = bad; s_first[tid >> 6] = first; s_slow[tid >> 6] = slow; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < RT / 64; ++w) { samples += s_samples[w]; bad += s_bad[w]; first = min(first, s_first[w]); slow += s_slow[w]; }
        d2d_flac_check c;
        c.samples_checked = samples; c.blocks_checked = fd.blocks; c.bad_blocks = bad; c.first_bad_block = first;
        c.first_bad_reason = bad ? status(first) & 0xFFu : (uint32_t)D2D_FLAC_BAD_NONE;
        *fd.check = c;
        if (fd.stats) {
            if (a.serial) slow = fd.blocks;
            d2d_flac_verify_stats st;
            st.fast_blocks = fd.blocks - slow; st.fallback_blocks = slow;
            *fd.stats = st;
        }
    }
}

// the cooperative kernel's dynamic LDS above the default limit: hipFuncSetAttribute acts on the current device, remembered per device
hipError_t launch_coop(const VerifyArgs& a, uint32_t max_blocks, uint32_t nf, hipStream_t s) {
    static std::mutex mu;
    static size_t allowed[64] = {};
    const size_t lds = coop_image_bytes(a.bound);
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if (dev < 0 || dev >= 64) return hipErrorInvalidDevice;
    {
        std::lock_guard<std::mutex> g(mu);
        if (allowed[dev] < lds) {
            e = hipFuncSetAttribute(reinterpret_cast<const void*>(&flac_verify_coop_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            if (e != hipSuccess) return e;
            allowed[dev] = lds;
        }
    }
    hipLaunchKernelGGL(flac_verify_coop_kernel, dim3(max_blocks, nf), dim3(NT), lds, s, a);
    return hipGetLastError();
}

}  // namespace

extern "C" int d2d_flac_verify_device(uint32_t channels, uint32_t bit_depth, const d2d_flac_io* io, uint32_t n_files,
                                      void* workspace, size_t workspace_bytes, d2d_flac_check* checks, void* hip_stream) {
    return d2d_flac_verify_device_method(channels, bit_depth, D2D_FLAC_VERIFY_AUTO, io, n_files, workspace, workspace_bytes, checks, nullptr, hip_stream);
}

extern "C" int d2d_flac_verify_device_method(uint32_t channels, uint32_t bit_depth, uint32_t method, const d2d_flac_io* io, uint32_t n_files,
                                             void* workspace, size_t workspace_bytes, d2d_flac_check* checks, d2d_flac_verify_stats* stats,
                                             void* hip_stream) {
    // every check comes before the first device call
    if (!verify_method_ok(method)) return fail(D2D_ERR_PARAM, VERIFY_METHOD_MESSAGE);
    if ((uintptr_t)stats & 3) return fail(D2D_ERR_PARAM, "stats must be null or a 4-byte aligned pointer the GPU can address");
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
        a.serial = method == D2D_FLAC_VERIFY_SERIAL;
        uint32_t max_blocks = 0;
        for (uint32_t i = 0; i < nf; ++i) {                         // the workspace is walked as the encode call walked it
            const d2d_flac_io& x = io[f0 + i];
            const size_t blocks = block_count(x.frames, x.final);
            VerifyFile& d = a.f[i];
            d.pcm = (const uint8_t*)x.pcm; d.out = (const uint8_t*)x.out; d.result = x.result; d.check = checks + f0 + i; d.stats = stats ? stats + f0 + i : nullptr;
            d.sizes = (const uint32_t*)ws; d.slots = ws + align16(4 * blocks);
            d.blocks = (uint32_t)blocks; d.first_block = x.first_block;
            d.last_n = (x.final && x.frames % BS) ? (uint32_t)(x.frames % BS) : BS;
            ws += d2d_flac_workspace_bytes(channels, bit_depth, x.frames, x.final);
            max_blocks = std::max(max_blocks, d.blocks);
        }
        if (max_blocks && a.serial) {
            hipLaunchKernelGGL(flac_verify_status_kernel, dim3((max_blocks + FPW - 1) / FPW, nf), dim3(VT), 0, s, a);
            const hipError_t e = hipGetLastError();
            if (e != hipSuccess) return hip_fail(e, "flac_verify_status_kernel");
        } else if (max_blocks) {
            const hipError_t e = launch_coop(a, max_blocks, nf, s);
            if (e != hipSuccess) return hip_fail(e, "flac_verify_coop_kernel");
        }
        hipLaunchKernelGGL(flac_verify_reduce_kernel, dim3(nf), dim3(RT), 0, s, a);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return hip_fail(e, "flac_verify_reduce_kernel");
    }
    return D2D_OK;
}
