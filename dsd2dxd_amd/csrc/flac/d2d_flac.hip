// d2d_flac.hip -- FLAC frames on the GPU (gfx950): the kernels behind d2d_flac_encode_device (the whole-stream driver on top of the
// public calls is d2d_flac_stream.cpp).  The bitstream is the one flac_frame_enc.h defines, at every effort; tests/test_gpu_flac.py
// (effort 0), tests/test_gpu_flac_search.py (effort 1) and tests/test_gpu_flac_lpc.py (effort 12) compare them byte for byte.  The
// rules' small arithmetic (Rice parameter, zigzag, pmax, header bit counts, the LPC routine) is flac_lpc.h, the host encoder's copy.
// Both encode kernels are a front of their own (PCM in LDS, the decisions, every thread's code lengths) and one emit path:
// block_context in front of everything, then scan_starts, begin_image, put_bits / put_rice and finish_frame (steps 3 to 6 below).
// The helpers the cooperative verify kernel (d2d_flac_verify.hip) needs as well -- put_bits, frame_crc16, scan_starts, the DPP sums and the
// workgroup's shape, NT and SPT -- live in flac_device.h.
//   flac_encode_kernel<CH>   effort 0: one workgroup of 1024 threads per (file, block); thread t owns samples 4t .. 4t+3 of every channel.
//     1. the block's PCM comes into LDS with 16-byte loads (4096 * frame_bytes is a multiple of 16; a short block's tail by bytes)
//     2. residuals r = s[i] - 2 s[i-1] + s[i-2] stay in registers; sum |r| per channel is reduced over the workgroup (64-bit) and
//        thread c derives k[c]
//     3. code lengths, one exclusive scan per channel over the threads, channel c starting where channel c-1 ended: every bit
//        position of the frame is known before a bit is placed
//     4. the LDS that held the PCM is zeroed and becomes the frame image (big-endian 32-bit words); each code ORs in its stop bit and
//        its k low bits (ds_or_b32), the unary zeros are the fill, so arrival order cannot matter
//     5. CRC-16 in parallel: init 0 makes the CRC linear and blind to leading zeros, so the frame is treated as 1024 equal chunks
//        with zeros in front, every thread runs the table over its chunk, and a tree combines  crc(A|B) = crc(A) x^(8 len B) + crc(B)
//     6. the image goes to the block's workspace slot (16-byte stores), its size to the size table
//   flac_search_kernel<CH, LPC>   efforts 1 and 12: the same workgroup and steps 3 to 6, with the search in front of them (described at
//                            the kernel); LPC = true adds effort 12's linear predictors and changes nothing of the LPC = false code
//   flac_pack_kernel        per file, 32 blocks per workgroup: sums the sizes in front of its blocks, copies the slots to `out`
//                            contiguously; the first workgroup of a file writes the result record.
// The two run one after the other on the caller's stream.  No workgroup waits on another: no look-back, no flags, no spinning.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <mutex>
#include <vector>

#include "d2d_flac_internal.h"
#include "flac_device.h"
#include "flac_lpc.h"

using namespace d2dflac;
using namespace d2drice;

namespace {

constexpr int MAXF = 16;          // files per launch: their descriptors ride in the kernel arguments
constexpr int PT = 256;           // threads of a pack workgroup
constexpr uint32_t PB = 32;       // blocks per pack workgroup

struct FileDesc {
    const uint8_t* pcm;
    uint8_t* out;
    d2d_flac_result* result;
    uint32_t* sizes;              // workspace: one size per block
    uint8_t* slots;               // workspace: one slot per block
    uint32_t blocks, first_block, last_n, pad;      // last_n: samples of the last block (4096, or the short one)
};
struct FlacArgs {
    FileDesc f[MAXF];
    uint32_t depth, slot_bytes;
};

__device__ __forceinline__ uint32_t utf8_len(uint32_t v) { return v < 0x80 ? 1 : v < 0x800 ? 2 : v < 0x10000 ? 3 : v < 0x200000 ? 4 : v < 0x4000000 ? 5 : 6; }

// the frame header and its CRC-8 (x^8 + x^2 + x + 1); `assignment` is the channel-assignment nibble.  One thread.
__device__ __forceinline__ void build_header(uint8_t* s_hdr, uint32_t n, uint32_t assignment, uint32_t depth, uint32_t frame_no) {
    uint32_t p = 0;
    s_hdr[p++] = 0xFF; s_hdr[p++] = 0xF8;
    s_hdr[p++] = n == BS ? 0xC0 : 0x70;
    s_hdr[p++] = (uint8_t)((assignment << 4) | ((depth == 16 ? 4u : depth == 20 ? 5u : 6u) << 1));
    if (frame_no < 0x80) s_hdr[p++] = (uint8_t)frame_no;
    else {
        const int m = (int)utf8_len(frame_no) - 1;
        s_hdr[p++] = (uint8_t)(((0xFF00u >> (m + 1)) & 0xFFu) | (frame_no >> (6 * m)));
        for (int i = m - 1; i >= 0; --i) s_hdr[p++] = (uint8_t)(0x80u | ((frame_no >> (6 * i)) & 0x3Fu));
    }
    if (n != BS) { s_hdr[p++] = (uint8_t)((n - 1) >> 8); s_hdr[p++] = (uint8_t)(n - 1); }
    uint32_t c = 0;
    for (uint32_t i = 0; i < p; ++i) {
        c ^= s_hdr[i];
        for (int k2 = 0; k2 < 8; ++k2) c = (c & 0x80u) ? ((c << 1) ^ 0x07u) & 0xFFu : (c << 1) & 0xFFu;
    }
    s_hdr[p] = (uint8_t)c;
}

// the image (big-endian words) to its 16-byte aligned slot
__device__ __forceinline__ void store_frame(const uint32_t* img, uint8_t* slot, uint32_t out_vecs, uint32_t tid) {
    uint4* dst = reinterpret_cast<uint4*>(slot);
    for (uint32_t v = tid; v < out_vecs; v += NT) {
        uint4 w = reinterpret_cast<const uint4*>(img)[v];
        w.x = __builtin_bswap32(w.x); w.y = __builtin_bswap32(w.y); w.z = __builtin_bswap32(w.z); w.w = __builtin_bswap32(w.w);
        dst[v] = w;
    }
}

// ---- what both encode kernels share: the block's context in front, the emit path behind -------------------------------------

__device__ __forceinline__ Block block_context(const FileDesc& fd, uint32_t b, uint32_t depth) {
    Block B;
    B.n = b + 1 == fd.blocks ? fd.last_n : BS; B.depth = depth;
    B.tid = threadIdx.x; B.lane = B.tid & 63u; B.wave = B.tid >> 6; B.i0 = B.tid * SPT;
    B.frame_no = fd.first_block + b;
    B.hdr_bytes = 4 + utf8_len(B.frame_no) + (B.n != BS ? 2u : 0u) + 1;
    B.pmax = search_pmax(B.n);                      // (0 for an unsearched frame, n < 16)
    B.fsz = B.n >> B.pmax; B.pj0 = B.i0 / B.fsz; B.rem0 = B.i0 - B.pj0 * B.fsz;
    return B;
}

template <int CH>
struct EmitLds {                                    // the emit path's static LDS
    uint32_t wtot[NW][CH];
    uint16_t crc_tab[256], crc[NT];
    uint8_t hdr[16];
};

// Step 4's beginning: the LDS behind `img` zeroed for a frame of data_bytes and its CRC-16, the header bytes placed.  Every thread must
// have passed a barrier behind its last read of what lay there.  False, for the whole workgroup, for a frame beyond the slot: the bound of
// include/dsd2dxd_amd.h says there is none at any effort; one that broke it is dropped whole, size 0, not written past the image.
__device__ __forceinline__ bool begin_image(uint32_t* img, uint32_t data_bytes, uint32_t slot_bytes, uint32_t* size, const uint8_t* s_hdr, const Block B) {
    if (data_bytes + 2 > slot_bytes) { if (B.tid == 0) *size = 0; return false; }
    for (uint32_t w = B.tid; w < ((data_bytes + 2 + 15) >> 4) * 4 + 4; w += NT) img[w] = 0;
    __syncthreads();
    if (B.tid < B.hdr_bytes && s_hdr[B.tid]) put_bits(img, B.tid * 8, s_hdr[B.tid], 8);
    return true;
}
// the Rice code of u under k at bit p: q = u >> k zeros (the fill), the stop bit, k low bits; returns the bit behind it
__device__ __forceinline__ uint32_t put_rice(uint32_t* img, uint32_t p, uint32_t u, uint32_t k) {
    const uint32_t q = u >> k;
    put_bits(img, p + q, (1u << k) | (u & ((1u << k) - 1)), k + 1);
    return p + q + 1 + k;
}
// Steps 5 and 6, once every thread has placed its bits: the CRC-16 behind the data bytes, the image to the slot, the frame's size
template <int CH>
__device__ __forceinline__ void finish_frame(uint32_t* img, uint32_t data_bytes, EmitLds<CH>& s, uint8_t* slot, uint32_t* size, uint32_t tid) {
    __syncthreads();
    frame_crc16(img, data_bytes, s.crc_tab, s.crc, tid);
    store_frame(img, slot, (data_bytes + 2 + 15) >> 4, tid);
    if (tid == 0) *size = data_bytes + 2;
}

template <int CH>
__global__ __launch_bounds__(NT) void flac_encode_kernel(const FlacArgs a) {
    extern __shared__ __align__(16) unsigned char smem[];          // the block's PCM, then the frame image
    __shared__ unsigned long long s_wsum[NW][CH];
    __shared__ uint32_t s_k[CH];
    __shared__ EmitLds<CH> s_emit;

    const FileDesc& fd = a.f[blockIdx.y];
    const uint32_t b = blockIdx.x;
    if (b >= fd.blocks) return;                                     // (the whole workgroup)
    const Block B = block_context(fd, b, a.depth);
    const uint32_t n = B.n, depth = B.depth, tid = B.tid, i0 = B.i0, sb = depth == 16 ? 2u : 3u, fb = CH * sb;
    const bool fixed2 = n > 2;                                      // else the verbatim subframe: every sample a warm-up

    // 1. PCM -> LDS
    {
        const uint8_t* src = fd.pcm + (size_t)b * BS * fb;
        const uint32_t nbytes = n * fb, nvec = nbytes >> 4;
        for (uint32_t v = tid; v < nvec; v += NT) reinterpret_cast<uint4*>(smem)[v] = reinterpret_cast<const uint4*>(src)[v];
        for (uint32_t j = (nvec << 4) + tid; j < nbytes; j += NT) smem[j] = src[j];
    }
    build_crc_tab(s_emit.crc_tab, tid);
    if (tid == 0) build_header(s_emit.hdr, n, CH - 1, depth, B.frame_no);
    __syncthreads();

    // 2. samples -> residuals (warm-up and verbatim samples stay as they are), sum |r|
    int32_t val[CH][SPT];
    auto sample = [&](uint32_t i, uint32_t c) -> int32_t {
        const uint8_t* q = smem + (i * CH + c) * sb;
        int32_t v = sb == 2 ? (int32_t)(int16_t)(q[0] | (q[1] << 8)) : (int32_t)((uint32_t)(q[0] | (q[1] << 8) | (q[2] << 16)) << 8) >> 8;
        return depth == 20 ? v >> 4 : v;
    };
    unsigned long long asum[CH];
#pragma unroll
    for (int c = 0; c < CH; ++c) {
        int32_t s2 = i0 >= 2 && i0 - 2 < n ? sample(i0 - 2, c) : 0, s1 = i0 >= 1 && i0 - 1 < n ? sample(i0 - 1, c) : 0;
        uint32_t acc = 0;
#pragma unroll
        for (int j = 0; j < SPT; ++j) {
            const uint32_t i = i0 + j;
            const int32_t s0 = i < n ? sample(i, c) : 0;
            int32_t v = s0;
            if (i < n && i >= 2) {                                  // |r| <= 2^25
                v = s0 - 2 * s1 + s2;
                acc += (uint32_t)(v < 0 ? -v : v);
            }
            val[c][j] = v;
            s2 = s1; s1 = s0;
        }
        unsigned long long t = acc;
        for (int o = 32; o >= 1; o >>= 1) t += __shfl_xor(t, o, 64);
        asum[c] = t;
    }
    if (B.lane == 0) {
#pragma unroll
        for (int c = 0; c < CH; ++c) s_wsum[B.wave][c] = asum[c];
    }
    __syncthreads();
    if (tid < CH) {
        unsigned long long sum = 0;
        for (int w = 0; w < NW; ++w) sum += s_wsum[w][tid];
        s_k[tid] = rice_k(sum, fixed2 ? n - 2 : 1);
    }
    __syncthreads();

    // 3. code lengths (thread 0 holds whatever is no residual) and where every thread's bits begin
    uint32_t kk[CH], mine[CH], start[CH];
#pragma unroll
    for (int c = 0; c < CH; ++c) {
        kk[c] = s_k[c];
        uint32_t len = tid != 0 ? 0 : fixed2 ? fixed_header_bits(2, depth) + PARAM_BITS : SUBFRAME_BITS + n * depth;
#pragma unroll
        for (int j = 0; j < SPT; ++j)
            if (i0 + j < n && i0 + j >= 2) len += (zigzag(val[c][j]) >> kk[c]) + 1 + kk[c];
        mine[c] = len;
    }
    const uint32_t data_bytes = (scan_starts<CH>(start, mine, B.hdr_bytes * 8, s_emit.wtot, B) + 7) >> 3;

    // 4. the image: zero fill, then the bits that are one
    uint32_t* img = reinterpret_cast<uint32_t*>(smem);
    if (!begin_image(img, data_bytes, a.slot_bytes, &fd.sizes[b], s_emit.hdr, B)) return;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
        uint32_t p = start[c];
        if (tid == 0) { put_bits(img, p, fixed2 ? 0x14u : 0x02u, SUBFRAME_BITS); p += SUBFRAME_BITS; }   // 0 001010 0: fixed order 2; 0 000001 0: verbatim
#pragma unroll
        for (int j = 0; j < SPT; ++j) {
            const uint32_t i = i0 + j;
            if (i >= n) continue;
            if (i == 2) { put_bits(img, p, (1u << 9) | kk[c], METHOD_BITS + PARAM_BITS); p += METHOD_BITS + PARAM_BITS; }   // 01: 5-bit Rice parameters, 0000: one partition, k
            if (i < 2) {
                const uint32_t raw = (uint32_t)val[c][j] & ((1u << depth) - 1);
                if (raw) put_bits(img, p, raw, depth);
                p += depth;
            } else p = put_rice(img, p, zigzag(val[c][j]), kk[c]);
        }
    }

    // 5. CRC-16 over the data_bytes in front of it; 6. image -> slot
    finish_frame(img, data_bytes, s_emit, fd.slots + (size_t)b * a.slot_bytes, &fd.sizes[b], tid);
}

// ---- effort 1: the search of flac_frame_enc.h -------------------------------------------------------------------------------

constexpr int NP = 64;            // Rice partitions of a whole block at the finest partition order, 6: 64 samples, 16 lanes each

// The block's PCM into LDS as planar 32-bit samples, pcm[c * BS + i]: thread t unpacks its frames 4t .. 4t+3, which are CH * SB
// whole dwords of the source (the block begins 16-byte aligned), and writes one 16-byte vector per channel.  A short block's last,
// partial group goes byte by byte, so that nothing behind the n frames is read.  Samples from n on stay unwritten.
template <int CH, int SB>
__device__ __forceinline__ void load_planar_sb(int32_t* pcm, const uint8_t* src, uint32_t n, uint32_t depth, uint32_t tid) {
    constexpr int ND = CH * SB;                                     // dwords of four frames
    const uint32_t i0 = tid * SPT;
    if (i0 >= n) return;
    uint32_t w[ND];
    if (i0 + SPT <= n) {
#pragma unroll
        for (int d = 0; d < ND; ++d) w[d] = reinterpret_cast<const uint32_t*>(src)[tid * ND + d];
    } else {
        const uint32_t have = (n - i0) * CH * SB;
#pragma unroll
        for (int d = 0; d < ND; ++d) {
            uint32_t v = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) if ((uint32_t)(4 * d + k) < have) v |= (uint32_t)src[(size_t)tid * ND * 4 + 4 * d + k] << (8 * k);
            w[d] = v;
        }
    }
    auto byte = [&](int k) -> uint32_t { return (w[k >> 2] >> (8 * (k & 3))) & 0xFFu; };
#pragma unroll
    for (int c = 0; c < CH; ++c) {
        int32_t v[SPT];
#pragma unroll
        for (int j = 0; j < SPT; ++j) {
            const int k = (j * CH + c) * SB;
            v[j] = SB == 2 ? (int32_t)(int16_t)(byte(k) | (byte(k + 1) << 8)) : (int32_t)((byte(k) | (byte(k + 1) << 8) | (byte(k + 2) << 16)) << 8) >> 8;
            if (depth == 20) v[j] >>= 4;
        }
        *reinterpret_cast<int4*>(pcm + c * BS + i0) = make_int4(v[0], v[1], v[2], v[3]);
    }
}
template <int CH>
__device__ __forceinline__ void load_planar(int32_t* pcm, const uint8_t* src, uint32_t n, uint32_t depth, uint32_t tid) {
    if (depth == 16) load_planar_sb<CH, 2>(pcm, src, n, depth, tid);
    else load_planar_sb<CH, 3>(pcm, src, n, depth, tid);
}
// x[w] = sample i0 - 4 + w of candidate signal sg, 0 outside [0, n): a thread's four samples behind their four predecessors.
// sg is a channel, or for two channels 2 = mid, 3 = side.
template <int CH>
__device__ __forceinline__ void load_window(int32_t (&x)[8], const int32_t* pcm, uint32_t i0, uint32_t n, uint32_t sg) {
    const int32_t* q = pcm + (CH == 2 && sg >= 2 ? 0u : sg) * BS + i0;
    const int4 z = make_int4(0, 0, 0, 0);
    const int4 lo = i0 ? *reinterpret_cast<const int4*>(q - 4) : z, hi = *reinterpret_cast<const int4*>(q);
    x[0] = lo.x; x[1] = lo.y; x[2] = lo.z; x[3] = lo.w; x[4] = hi.x; x[5] = hi.y; x[6] = hi.z; x[7] = hi.w;
    if (CH == 2 && sg >= 2) {
        const int4 rlo = i0 ? *reinterpret_cast<const int4*>(q + BS - 4) : z, rhi = *reinterpret_cast<const int4*>(q + BS);
        const int32_t r[8] = {rlo.x, rlo.y, rlo.z, rlo.w, rhi.x, rhi.y, rhi.z, rhi.w};
#pragma unroll
        for (int w = 0; w < 8; ++w) x[w] = sg == 2 ? (x[w] + r[w]) >> 1 : x[w] - r[w];
    }
#pragma unroll
    for (int w = 4; w < 8; ++w) if (i0 + w - 4 >= n) x[w] = 0;      // (what lies before i0 lies below n, or nothing here is used)
}
// one more difference over the window: residuals of order o from those of order o - 1, in x[o ..]
__device__ __forceinline__ void difference(int32_t (&x)[8], int o) {
#pragma unroll
    for (int w = 7; w >= 1; --w) if (w >= o) x[w] -= x[w - 1];
}

// ---- effort 12: what the LPC flavour of the search kernel adds ----------------------------------------------------------------
// x[w] = sample i0 - 12 + w of candidate signal sg, 0 outside [0, n): a thread's four samples behind their twelve predecessors
template <int CH>
__device__ __forceinline__ void load_window16(int32_t (&x)[16], const int32_t* pcm, uint32_t i0, uint32_t n, uint32_t sg) {
    const int32_t* q = pcm + (CH == 2 && sg >= 2 ? 0u : sg) * BS + i0;
    const int4 z = make_int4(0, 0, 0, 0);
#pragma unroll
    for (int v = 0; v < 4; ++v) {
        const bool in = i0 + 4 * v >= 12;                           // (i0 is a multiple of 4: a vector lies wholly in front of sample 0 or not at all)
        int4 l = in ? *reinterpret_cast<const int4*>(q + 4 * v - 12) : z;
        if (CH == 2 && sg >= 2) {
            const int4 r = in ? *reinterpret_cast<const int4*>(q + BS + 4 * v - 12) : z;
            if (sg == 2) l = make_int4((l.x + r.x) >> 1, (l.y + r.y) >> 1, (l.z + r.z) >> 1, (l.w + r.w) >> 1);
            else l = make_int4(l.x - r.x, l.y - r.y, l.z - r.z, l.w - r.w);
        }
        x[4 * v] = l.x; x[4 * v + 1] = l.y; x[4 * v + 2] = l.z; x[4 * v + 3] = l.w;
    }
#pragma unroll
    for (int w = 12; w < 16; ++w) if (i0 + w - 12 >= n) x[w] = 0;   // (what lies before i0 lies below n, or nothing here is used)
}
// the four residuals of a thread's samples under 12 coefficients (a lower order's are zero from its order on)
__device__ __forceinline__ void lpc_residuals4(int32_t (&r)[SPT], const int32_t (&x)[16], const int32_t* s_q, int32_t shift) {
    int32_t q[d2dlpc::MAX_ORDER], rev[16];
#pragma unroll
    for (int j = 0; j < d2dlpc::MAX_ORDER; ++j) q[j] = s_q[j];
#pragma unroll
    for (int w = 0; w < 16; ++w) rev[w] = x[15 - w];                // rev[4 - j + m] = x(i0 + j - 1 - m)
#pragma unroll
    for (int j = 0; j < SPT; ++j) r[j] = d2dlpc::lpc_residual<d2dlpc::MAX_ORDER>(x[12 + j], &rev[4 - j], q, shift);
}
// a signed 64-bit sum over the wave, exact for |total| < 2^62, as three 32-bit sums of 22-bit limbs (the top one signed)
__device__ __forceinline__ long long wave_sum_i64(long long v) {
    const uint32_t lo = wave_sum((uint32_t)v & 0x3FFFFFu), mid = wave_sum((uint32_t)(v >> 22) & 0x3FFFFFu);
    const int32_t hi = (int32_t)wave_sum((uint32_t)(int32_t)(v >> 44));
    return (long long)(((unsigned long long)(long long)hi << 44) + ((unsigned long long)mid << 22) + lo);
}

// ---- the stages of the search kernel (the letters are those of its head comment) ------------------------------------------------

// row `which` of u, without indexing registers by a variable
template <int N>
__device__ __forceinline__ void pick(uint32_t (&out)[SPT], const uint32_t (&u)[N][SPT], uint32_t which) {
#pragma unroll
    for (int j = 0; j < SPT; ++j) {
        out[j] = u[0][j];
#pragma unroll
        for (int s = 1; s < N; ++s) if (which == (uint32_t)s) out[j] = u[s][j];
    }
}
// (a) and (h), the part they share: N residual sets of this thread's four samples as u = zigzag(r), set s coded from sample
// FIRST + STEP s on; len[s] = the exact length of its codes under one k, that of its sum |r| = sum (u + 1) >> 1: one N-wide 64-bit
// reduction (|r| < 2^30: below 2^48), threads 0 .. N-1 derive the N k, one N-wide reduction of the lengths.
template <int N, int FIRST, int STEP>
__device__ __forceinline__ void rice_costs(uint32_t (&len)[N], const uint32_t (&u)[N][SPT], const Block B, uint32_t* s_ko, unsigned long long* s_red) {
    auto coded = [&](int s, int j) -> bool { return B.i0 + j < B.n && B.i0 + j >= (uint32_t)(FIRST + STEP * s); };
    unsigned long long sum[N];
#pragma unroll
    for (int s = 0; s < N; ++s) {
        sum[s] = 0;
#pragma unroll
        for (int j = 0; j < SPT; ++j) if (coded(s, j)) sum[s] += (u[s][j] + 1) >> 1;
    }
    wg_sum<N>(sum, s_red, B.lane, B.wave);
    if (B.tid < (uint32_t)N) {
        unsigned long long mine = sum[0];
#pragma unroll
        for (int s = 1; s < N; ++s) if (B.tid == (uint32_t)s) mine = sum[s];
        const uint32_t first = FIRST + STEP * B.tid;
        s_ko[B.tid] = rice_k(mine, B.n > first ? B.n - first : 1);
    }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < N; ++s) {
        const uint32_t k = s_ko[s];
        len[s] = 0;
#pragma unroll
        for (int j = 0; j < SPT; ++j) if (coded(s, j)) len[s] += (u[s][j] >> k) + 1 + k;
    }
    wg_sum<N>(len, s_red, B.lane, B.wave);
}
// (a) for signal sg of `bits` bits: the fixed order with the least exact cost at one partition, the smallest at a tie (rule 5); an
// unsearched frame (n < 16) gets effort 0's: order 2, or verbatim (every sample a warm-up).  uo = that order's residuals.
template <int CH>
__device__ __forceinline__ uint32_t fixed_order(uint32_t (&uo)[SPT], uint32_t bits, const int32_t* pcm, const Block B, uint32_t sg, uint32_t* s_ko, unsigned long long* s_red) {
    uint32_t u[5][SPT], len[5], order = 0, cost = 0;
    int32_t x[8];
    load_window<CH>(x, pcm, B.i0, B.n, sg);
#pragma unroll
    for (int o = 0; o < 5; ++o) {
        if (o) difference(x, o);
#pragma unroll
        for (int j = 0; j < SPT; ++j) u[o][j] = zigzag(x[4 + j]);
    }
    rice_costs<5, 0, 1>(len, u, B, s_ko, s_red);
#pragma unroll
    for (int o = 0; o < 5; ++o) {
        const uint32_t c = fixed_header_bits(o, bits) + PARAM_BITS + len[o];
        if (o == 0 || c < cost) { order = o; cost = c; }
    }
    if (B.n < 16) order = B.n > 2 ? 2u : B.n;
    pick<5>(uo, u, order);
    return order;
}
// (h): the candidate of `valid` (not 0) with the least exact cost at one partition, the smaller order at a tie (rule 16); its
// residuals, 64-bit multiply-adds from the PCM plane, in uo
template <int CH>
__device__ __forceinline__ uint32_t lpc_order(uint32_t (&uo)[SPT], uint32_t bits, uint32_t valid, const d2dlpc::LpcCoefs& s_cand, const int32_t* pcm, const Block B,
                                              uint32_t sg, uint32_t* s_ko, unsigned long long* s_red) {
    using namespace d2dlpc;
    uint32_t u[CANDIDATES][SPT], len[CANDIDATES], best = 0, cost = 0;
    int32_t xw[16];
    load_window16<CH>(xw, pcm, B.i0, B.n, sg);
#pragma unroll
    for (int c = 0; c < CANDIDATES; ++c) {                          // (a candidate that does not exist: zeros, its cost unused)
        int32_t r[SPT] = {0, 0, 0, 0};
        if (valid >> c & 1u) lpc_residuals4(r, xw, s_cand.q[c], s_cand.shift[c]);
#pragma unroll
        for (int j = 0; j < SPT; ++j) u[c][j] = zigzag(r[j]);
    }
    rice_costs<CANDIDATES, 4, 4>(len, u, B, s_ko, s_red);
    bool any = false;
#pragma unroll
    for (int c = 0; c < CANDIDATES; ++c) {
        const uint32_t cc = lpc_header_bits(4 * (c + 1), bits) + PARAM_BITS + len[c];
        if ((valid >> c & 1u) && (!any || cc < cost)) { any = true; best = c; cost = cc; }
    }
    pick<CANDIDATES>(uo, u, best);
    return best;
}
// (b) and (c) for one residual set uo of predictor order `order` with hdrbits in front of its partitions: the partition order and
// the subframe's exact cost.  s_psum must be zero, a barrier passed since; s_kt keeps the k of every partition of every order.
struct Partitions { uint32_t porder, cost; };
__device__ __forceinline__ Partitions partition_search(const uint32_t (&uo)[SPT], uint32_t order, uint32_t hdrbits, const Block B,
                                                       unsigned long long* s_psum, uint8_t* s_kt, unsigned long long* s_red) {
    const uint32_t n = B.n, i0 = B.i0, tid = B.tid;
    // (b) sum |r| per finest partition, then k for every partition of every order
    if (n == BS) {                                                  // 16 lanes hold one partition
        unsigned long long t = 0;
#pragma unroll
        for (int j = 0; j < SPT; ++j) if (i0 + j >= order) t += (uo[j] + 1) >> 1;
        t = row_sum(t);
        if ((B.lane & 15u) == 0) s_psum[tid >> 4] = t;
    } else {
        unsigned long long run = 0;
        uint32_t pj = B.pj0, rem = B.rem0;
#pragma unroll
        for (int j = 0; j < SPT; ++j) {
            if (i0 + j < n && i0 + j >= order) run += (uo[j] + 1) >> 1;
            const bool ends = j == SPT - 1 || rem + 1 == B.fsz;
            if (ends && run) { atomicAdd(&s_psum[pj], run); run = 0; }         // (run != 0 only below n: pj < 2^pmax)
            if (++rem == B.fsz) { rem = 0; ++pj; }
        }
    }
    __syncthreads();
    if (tid < 2 * NP - 1) {
        const uint32_t p = 31u - (uint32_t)__clz(tid + 1), j = tid + 1 - (1u << p);
        if (p <= B.pmax) {
            const uint32_t span = 1u << (B.pmax - p);
            unsigned long long sum = 0;
            for (uint32_t t = 0; t < span; ++t) sum += s_psum[j * span + t];
            s_kt[tid] = (uint8_t)rice_k(sum, (n >> p) - (j == 0 ? order : 0u));
        }
    }
    __syncthreads();

    // (c) the cost of every partition order
    uint32_t plen[7];
#pragma unroll
    for (int p = 0; p < 7; ++p) plen[p] = 0;
    uint32_t pj = B.pj0, rem = B.rem0;
#pragma unroll
    for (int j = 0; j < SPT; ++j) {
        if (i0 + j < n && i0 + j >= order) {
#pragma unroll
            for (int p = 0; p < 7; ++p)
                if ((uint32_t)p <= B.pmax) { const uint32_t k = s_kt[(1u << p) - 1 + (pj >> (B.pmax - p))]; plen[p] += (uo[j] >> k) + 1 + k; }
        }
        if (++rem == B.fsz) { rem = 0; ++pj; }
    }
    wg_sum<7>(plen, s_red, B.lane, B.wave);
    Partitions best = {0, hdrbits + PARAM_BITS + plen[0]};
#pragma unroll
    for (int p = 1; p < 7; ++p) {                                   // the smallest partition order wins a tie
        const uint32_t c = hdrbits + (PARAM_BITS << p) + plen[p];
        if ((uint32_t)p <= B.pmax && c < best.cost) { best.porder = p; best.cost = c; }
    }
    return best;
}
// (f) and (g) for signal sg: the windowed signal into yplane; R(0 .. 12) from every thread's four y and their twelve predecessors by
// three-limb wave sums and 64-bit LDS adds (exact, whatever the order of arrival); thread 0 runs flac_lpc.h from R to the candidates in
// s_cand (coefficients zero from their order on), the others wait at the barrier.  Returns the valid mask.
template <int CH>
__device__ __forceinline__ uint32_t lpc_candidates(d2dlpc::LpcCoefs& s_cand, unsigned long long* s_R, int32_t* yplane, const int32_t* pcm, const Block B, uint32_t sg) {
    using namespace d2dlpc;
    const uint32_t n = B.n, i0 = B.i0;
    {
        int32_t xw[16];
        load_window16<CH>(xw, pcm, i0, n, sg);
        const uint32_t ws = lpc_window_shift(n);
        int32_t y[SPT];
#pragma unroll
        for (int j = 0; j < SPT; ++j) y[j] = i0 + j < n ? lpc_window(xw[12 + j], i0 + j, n, ws) : 0;
        *reinterpret_cast<int4*>(yplane + i0) = make_int4(y[0], y[1], y[2], y[3]);
    }
    if (B.tid <= (uint32_t)MAX_ORDER) s_R[B.tid] = 0;
    __syncthreads();
    {
        int32_t yw[16];
        const int4 z = make_int4(0, 0, 0, 0);
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int4 l = i0 + 4 * v >= 12 ? *reinterpret_cast<const int4*>(yplane + i0 + 4 * v - 12) : z;
            yw[4 * v] = l.x; yw[4 * v + 1] = l.y; yw[4 * v + 2] = l.z; yw[4 * v + 3] = l.w;
        }
#pragma unroll
        for (int l = 0; l <= MAX_ORDER; ++l) {
            long long part = 0;                                     // |y| <= 2^24: a thread's part stays below 2^50, a wave's below 2^56
#pragma unroll
            for (int j = 0; j < SPT; ++j) part += (long long)yw[12 + j] * yw[12 + j - l];
            part = wave_sum_i64(part);
            if (B.lane == 0) atomicAdd(&s_R[l], (unsigned long long)part);
        }
    }
    __syncthreads();
    if (B.tid == 0) {
        int64_t R[MAX_ORDER + 1];
#pragma unroll
        for (int l = 0; l <= MAX_ORDER; ++l) R[l] = (int64_t)s_R[l];
        LpcCoefs co;
        lpc_coefficients(R, co);
#pragma unroll
        for (int c = 0; c < CANDIDATES; ++c) {
            if (!(co.valid >> c & 1u)) continue;
#pragma unroll
            for (int j = 0; j < MAX_ORDER; ++j) s_cand.q[c][j] = j < 4 * (c + 1) ? co.q[c][j] : 0;
            s_cand.shift[c] = co.shift[c];
        }
        s_cand.valid = co.valid;
    }
    __syncthreads();
    return s_cand.valid;
}

//   flac_search_kernel<CH, LPC>   the same workgroup, with the decisions of effort 1 between "PCM in LDS" and "place bits".  Candidate
//   signals (the channels; for two channels also mid and side) go through their stages one at a time, so that one signal's five
//   residual sets are all the registers hold:
//     (a) fixed_order, (b) and (c) partition_search: the signal's effort-1 plan; the chosen partition order's k row is kept per signal
//     LPC (effort 12, rules 9 to 19 of flac_frame_enc.h; frames of 64 samples and more): (f) and (g) lpc_candidates, (h) lpc_order,
//     (i) partition_search once more; the signal keeps its effort-1 plan unless this one is strictly cheaper
//     (d) two channels: the assignment from the four signals' costs
//     (e) per subframe the chosen signal's residuals again (an LPC subframe's from the kept coefficients), now kept; lengths with the
//         residual header in front of sample `order` and a 5-bit k in front of every partition's first residual; then the emit path.
//   A frame of fewer than 16 samples takes the same path with the choices forced to effort 0's.
struct Plan { uint32_t order, porder, cost; };                      // what (a) to (c), or (f) to (i), chose for a signal
struct KeptLpc { int32_t q[d2dlpc::MAX_ORDER], shift; uint32_t lpc; };      // a signal's coefficients (zero from its order on), and whether its plan is LPC

template <int CH, bool LPC>
__global__ __launch_bounds__(NT) void flac_search_kernel(const FlacArgs a) {
    using namespace d2dlpc;
    constexpr int NSIG = CH == 2 ? 4 : CH;
    extern __shared__ __align__(16) unsigned char smem[];          // the block's PCM as planar 32-bit samples, then the frame image
    __shared__ unsigned long long s_red[NW * 8];
    __shared__ unsigned long long s_psum[NP];
    __shared__ uint32_t s_ko[5];
    __shared__ Plan s_plan[NSIG];
    __shared__ uint8_t s_kt[2 * NP];                                // k of partition j at partition order p: s_kt[2^p - 1 + j]
    __shared__ uint8_t s_ksel[NSIG][NP];                            // ... the chosen order's row
    __shared__ KeptLpc s_lpc[LPC ? NSIG : 1];                       // (without LPC a placeholder)
    __shared__ EmitLds<CH> s_emit;

    const FileDesc& fd = a.f[blockIdx.y];
    const uint32_t b = blockIdx.x;
    if (b >= fd.blocks) return;                                     // (the whole workgroup)
    const Block B = block_context(fd, b, a.depth);
    const uint32_t n = B.n, depth = B.depth, tid = B.tid, i0 = B.i0, pmax = B.pmax, fsz = B.fsz;
    const bool searched = n >= 16;

    int32_t* pcm = reinterpret_cast<int32_t*>(smem);
    int32_t* yplane = pcm + CH * BS;                                // (LPC only: the launch asks for it)
    load_planar<CH>(pcm, fd.pcm + (size_t)b * BS * CH * (depth == 16 ? 2u : 3u), n, depth, tid);
    build_crc_tab(s_emit.crc_tab, tid);
    __syncthreads();

    // a signal's plan and the k row of its partition order, which the partition search has just left in s_kt
    auto keep = [&](uint32_t sg, uint32_t order, Partitions part, bool lpc) {
        if (tid == 0) { s_plan[sg] = Plan{order, part.porder, part.cost}; if (LPC) s_lpc[sg].lpc = lpc; }
        if (tid < (1u << part.porder)) s_ksel[sg][tid] = s_kt[(1u << part.porder) - 1 + tid];
    };
#pragma unroll 1
    for (uint32_t sg = 0; sg < (uint32_t)NSIG; ++sg) {
        const uint32_t bits = CH == 2 && sg == 3 ? depth + 1 : depth;
        // the effort-1 plan (rules 3 to 6): (a) the predictor order, (b) and (c) its partition order
        if (tid < NP) s_psum[tid] = 0;                              // (read last before the barriers of the previous plan's sums)
        uint32_t uo[SPT];
        const uint32_t order = fixed_order<CH>(uo, bits, pcm, B, sg, s_ko, s_red);
        const Partitions fixed = partition_search(uo, order, fixed_header_bits(order, bits), B, s_psum, s_kt, s_red);
        keep(sg, order, fixed, false);

        // the LPC plan (rules 11 to 16): (f) and (g) the candidates, (h) the order, (i) its partition order; it replaces the effort-1
        // plan only where it is strictly cheaper (rule 17)
        if constexpr (LPC) {
            __shared__ unsigned long long s_R[MAX_ORDER + 1];
            __shared__ LpcCoefs s_cand;
            if (n < MIN_FRAME) continue;
            if (tid < NP) s_psum[tid] = 0;                          // (read last before the barriers of the effort-1 plan's sums)
            const uint32_t valid = lpc_candidates<CH>(s_cand, s_R, yplane, pcm, B, sg);
            if (!valid) continue;
            const uint32_t best = lpc_order<CH>(uo, bits, valid, s_cand, pcm, B, sg, s_ko, s_red), P = 4 * (best + 1);
            const Partitions lpc = partition_search(uo, P, lpc_header_bits(P, bits), B, s_psum, s_kt, s_red);
            if (!(lpc.cost < fixed.cost)) continue;
            if (tid < (uint32_t)MAX_ORDER) s_lpc[sg].q[tid] = s_cand.q[best][tid];
            if (tid == 0) s_lpc[sg].shift = s_cand.shift[best];
            keep(sg, P, lpc, true);
        }
    }
    __syncthreads();

    // (d) the channel assignment: independent, left/side, side/right, mid/side; ties in this order
    uint32_t mode = 0;
    if (CH == 2 && searched) {
        const uint32_t L = s_plan[0].cost, R = s_plan[1].cost, M = s_plan[NSIG > 2 ? 2 : 0].cost, S = s_plan[NSIG > 3 ? 3 : 0].cost;
        uint32_t total = L + R;
        if (L + S < total) { total = L + S; mode = 1; }
        if (S + R < total) { total = S + R; mode = 2; }
        if (M + S < total) { total = M + S; mode = 3; }
    }
    if (tid == 0) build_header(s_emit.hdr, n, mode == 0 ? CH - 1 : 7 + mode, depth, B.frame_no);
    auto subframe_signal = [&](int c) -> uint32_t {
        if (CH != 2) return (uint32_t)c;
        return c == 0 ? (mode == 2 ? 3u : mode == 3 ? 2u : 0u) : (mode == 0 || mode == 2 ? 1u : 3u);
    };

    // (e) the chosen residuals (warm-up samples as they are), code lengths, and where every thread's bits begin
    int32_t val[CH][SPT];
    uint32_t mine[CH], start[CH];
#pragma unroll
    for (int c = 0; c < CH; ++c) {
        const uint32_t sg = subframe_signal(c), order = s_plan[sg].order, sh = pmax - s_plan[sg].porder;
        const uint32_t bits = CH == 2 && sg == 3 ? depth + 1 : depth;
        const bool lp = LPC && s_lpc[LPC ? sg : 0].lpc;
        int32_t x[8], raw[SPT];
        if (LPC && lp) {
            int32_t xw[16], r[SPT];
            load_window16<CH>(xw, pcm, i0, n, sg);
            lpc_residuals4(r, xw, s_lpc[sg].q, s_lpc[sg].shift);
#pragma unroll
            for (int j = 0; j < SPT; ++j) { raw[j] = xw[12 + j]; x[4 + j] = r[j]; }
        } else {
            load_window<CH>(x, pcm, i0, n, sg);
#pragma unroll
            for (int j = 0; j < SPT; ++j) raw[j] = x[4 + j];
#pragma unroll
            for (int o = 1; o < 5; ++o) if ((uint32_t)o <= order) difference(x, o);
        }
        uint32_t len = tid == 0 ? SUBFRAME_BITS : 0;
        uint32_t pj = B.pj0, rem = B.rem0;
#pragma unroll
        for (int j = 0; j < SPT; ++j) {
            const uint32_t i = i0 + j;
            val[c][j] = i < order ? raw[j] : x[4 + j];
            if (i < n) {
                if (i < order) len += bits;
                else {
                    if (i == order) len += METHOD_BITS;             // 01 pppp
                    if (LPC && lp && i == order) len += lpc_coef_bits(order);     // 1101 sssss and the coefficients
                    if (i == order || (rem == 0 && (pj & ((1u << sh) - 1)) == 0)) len += PARAM_BITS;     // a partition's first residual: kkkkk
                    const uint32_t k = s_ksel[sg][pj >> sh];
                    len += (zigzag(val[c][j]) >> k) + 1 + k;
                }
            }
            if (++rem == fsz) { rem = 0; ++pj; }
        }
        mine[c] = len;
    }
    const uint32_t data_bytes = (scan_starts<CH>(start, mine, B.hdr_bytes * 8, s_emit.wtot, B) + 7) >> 3;

    // the image: zero fill, then the bits that are one
    uint32_t* img = reinterpret_cast<uint32_t*>(smem);
    if (!begin_image(img, data_bytes, a.slot_bytes, &fd.sizes[b], s_emit.hdr, B)) return;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
        const uint32_t sg = subframe_signal(c), order = s_plan[sg].order, porder = s_plan[sg].porder, sh = pmax - porder;
        const uint32_t bits = CH == 2 && sg == 3 ? depth + 1 : depth;
        const bool lp = LPC && s_lpc[LPC ? sg : 0].lpc;
        uint32_t p = start[c];
        if (tid == 0) {                                             // 0 1ppppp 0: LPC order ppppp + 1; 0 001ooo 0: fixed order ooo; 0 000001 0: verbatim
            put_bits(img, p, LPC && lp ? (0x20u | (order - 1)) << 1 : n > 2 ? (8u | order) << 1 : 0x02u, SUBFRAME_BITS);
            p += SUBFRAME_BITS;
        }
        uint32_t pj = B.pj0, rem = B.rem0;
#pragma unroll
        for (int j = 0; j < SPT; ++j) {
            const uint32_t i = i0 + j;
            if (i < n) {
                if (i < order) {
                    const uint32_t raw = (uint32_t)val[c][j] & (0xFFFFFFFFu >> (32 - bits));
                    if (raw) put_bits(img, p, raw, bits);
                    p += bits;
                } else {
                    const uint32_t k = s_ksel[sg][pj >> sh];
                    if (LPC && lp && i == order) {                  // 1101: 14-bit coefficients; their shift; the coefficients
                        put_bits(img, p, ((uint32_t)(PRECISION - 1) << 5) | (uint32_t)s_lpc[sg].shift, 9); p += 9;
                        for (uint32_t m = 0; m < order; ++m) { put_bits(img, p, (uint32_t)s_lpc[sg].q[m] & 0x3FFFu, PRECISION); p += PRECISION; }
                    }
                    if (i == order) { put_bits(img, p, (1u << 4) | porder, METHOD_BITS); p += METHOD_BITS; }      // 01: 5-bit Rice parameters, pppp
                    if (i == order || (rem == 0 && (pj & ((1u << sh) - 1)) == 0)) { if (k) put_bits(img, p, k, PARAM_BITS); p += PARAM_BITS; }
                    p = put_rice(img, p, zigzag(val[c][j]), k);
                }
            }
            if (++rem == fsz) { rem = 0; ++pj; }
        }
    }
    finish_frame(img, data_bytes, s_emit, fd.slots + (size_t)b * a.slot_bytes, &fd.sizes[b], tid);
}

// sum, min and max of sizes[lo, hi) over the workgroup; every thread gets them
__device__ void pack_reduce(const uint32_t* sizes, uint32_t lo, uint32_t hi, unsigned long long* red, unsigned long long& sum, uint32_t& mn, uint32_t& mx) {
    unsigned long long s = 0; uint32_t a = 0xFFFFFFFFu, z = 0;
    for (uint32_t i = lo + threadIdx.x; i < hi; i += PT) { const uint32_t v = sizes[i]; s += v; a = min(a, v); z = max(z, v); }
    for (int o = 32; o >= 1; o >>= 1) { s += __shfl_xor(s, o, 64); a = min(a, (uint32_t)__shfl_xor(a, o, 64)); z = max(z, (uint32_t)__shfl_xor(z, o, 64)); }
    const uint32_t wave = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) { red[wave * 3] = s; red[wave * 3 + 1] = a; red[wave * 3 + 2] = z; }
    __syncthreads();
    sum = 0; mn = 0xFFFFFFFFu; mx = 0;
    for (int w = 0; w < PT / 64; ++w) { sum += red[w * 3]; mn = min(mn, (uint32_t)red[w * 3 + 1]); mx = max(mx, (uint32_t)red[w * 3 + 2]); }
}

__global__ __launch_bounds__(PT) void flac_pack_kernel(const FlacArgs a) {
    __shared__ unsigned long long red[3 * PT / 64];
    const FileDesc& fd = a.f[blockIdx.y];
    const uint32_t b0 = blockIdx.x * PB, tid = threadIdx.x;
    if (blockIdx.x != 0 && b0 >= fd.blocks) return;
    unsigned long long off; uint32_t mn, mx;
    if (blockIdx.x == 0) {                                          // the record: this workgroup starts at offset 0 anyway
        pack_reduce(fd.sizes, 0, fd.blocks, red, off, mn, mx);
        if (tid == 0) { d2d_flac_result r; r.bytes_out = off; r.min_frame_bytes = fd.blocks ? mn : 0; r.max_frame_bytes = mx; *fd.result = r; }
        off = 0;
    } else pack_reduce(fd.sizes, 0, b0, red, off, mn, mx);
    const uint32_t b1 = min(b0 + PB, fd.blocks);
    for (uint32_t b = b0; b < b1; ++b) {
        const uint32_t size = fd.sizes[b];
        const uint8_t* src = fd.slots + (size_t)b * a.slot_bytes;    // 16-byte aligned
        uint8_t* dst = fd.out + off;
        // bytes up to dst's next 4-byte boundary, whole words put together from two source words, the last bytes: exactly [off, off + size)
        const uint32_t h = min((4u - (uint32_t)(off & 3u)) & 3u, size);
        if (tid < h) dst[tid] = src[tid];
        const uint32_t nw = (size - h) >> 2, sh = 8 * h;
        const uint32_t* s32 = reinterpret_cast<const uint32_t*>(src);
        uint32_t* d32 = reinterpret_cast<uint32_t*>(dst + h);
        for (uint32_t m = tid; m < nw; m += PT) {
            uint32_t w = s32[m];
            if (h) w = (w >> sh) | (s32[m + 1] << (32 - sh));       // (word m + 1 begins below `size`: the code needs its first h bytes)
            d32[m] = w;
        }
        for (uint32_t j = h + 4 * nw + tid; j < size; j += PT) dst[j] = src[j];
        off += size;
    }
}

enum class Encoder { fixed2, search, search_lpc };                  // flac_encode_kernel; flac_search_kernel<CH, false>; flac_search_kernel<CH, true>

// the frame image over the block's PCM: packed as it comes at effort 0, planar 32-bit samples in the search kernel, whose LPC flavour
// keeps the windowed signal's plane behind them
size_t encode_lds_bytes(uint32_t ch, uint32_t depth, Encoder enc) {
    const size_t pcm = (size_t)BS * ch * (enc == Encoder::fixed2 ? sample_bytes(depth) : 4) + (enc == Encoder::search_lpc ? (size_t)BS * 4 : 0);
    return std::max<size_t>(slot_bytes(ch, depth) + 32, pcm);
}

template <int CH, Encoder ENC>
hipError_t launch_encode(const FlacArgs& a, uint32_t max_blocks, uint32_t nf, hipStream_t s) {
    const auto kernel = ENC == Encoder::fixed2 ? &flac_encode_kernel<CH> : ENC == Encoder::search ? &flac_search_kernel<CH, false> : &flac_search_kernel<CH, true>;
    // hipFuncSetAttribute acts on the current device: remembered per device, under a lock
    static std::mutex mu;
    static size_t allowed[64] = {};
    const size_t lds = encode_lds_bytes(CH, a.depth, ENC);
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if (dev < 0 || dev >= 64) return hipErrorInvalidDevice;
    {
        std::lock_guard<std::mutex> g(mu);
        if (allowed[dev] < lds) {
            e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            if (e != hipSuccess) return e;
            allowed[dev] = lds;
        }
    }
    hipLaunchKernelGGL(kernel, dim3(max_blocks, nf), dim3(NT), lds, s, a);
    return hipGetLastError();
}

template <Encoder ENC, int CH = 8>                                  // ch = 1 .. 8 to launch_encode<ch, ENC>
hipError_t launch_encode_ch(uint32_t ch, const FlacArgs& a, uint32_t max_blocks, uint32_t nf, hipStream_t s) {
    if constexpr (CH > 1) if (ch < (uint32_t)CH) return launch_encode_ch<ENC, CH - 1>(ch, a, max_blocks, nf, s);
    return launch_encode<CH, ENC>(a, max_blocks, nf, s);
}

}  // namespace

int d2dflac::hip_fail(hipError_t e, const char* what) { return fail(D2D_ERR_DEVICE, std::string(what) + ": " + hipGetErrorString(e)); }

extern "C" {

int d2d_flac_encode_device(uint32_t channels, uint32_t bit_depth, d2d_flac_io* io, uint32_t n_files,
                           void* workspace, size_t workspace_bytes, void* hip_stream) {
    return d2d_flac_encode_device_effort(channels, bit_depth, D2D_FLAC_EFFORT_FIXED2, io, n_files, workspace, workspace_bytes, hip_stream);
}

int d2d_flac_encode_device_effort(uint32_t channels, uint32_t bit_depth, uint32_t effort, d2d_flac_io* io, uint32_t n_files,
                                  void* workspace, size_t workspace_bytes, void* hip_stream) {
    // every check comes before the first device call
    if (!effort_ok(effort)) return fail(D2D_ERR_PARAM, EFFORT_MESSAGE);
    if (!depth_ok(bit_depth)) return fail(D2D_ERR_PARAM, "FLAC holds 16, 20 or 24-bit integers (Invalid bit depth)");
    if (channels == 0 || channels > 8) return fail(D2D_ERR_PARAM, "FLAC holds 1 to 8 channels (Invalid channel count)");
    if (!io || n_files == 0) return fail(D2D_ERR_PARAM, "no files");
    size_t need = 0, any_blocks = 0;
    for (uint32_t f = 0; f < n_files; ++f) {
        const d2d_flac_io& x = io[f];
        const size_t blocks = block_count(x.frames, x.final);
        if ((uint64_t)x.first_block + blocks > (1ull << 31)) return fail(D2D_ERR_PARAM, "frame numbers are 31 bits: first_block + blocks exceeds 2^31");
        if (!x.result) return fail(D2D_ERR_PARAM, "null result record");
        if (((uintptr_t)x.pcm & 15) || ((uintptr_t)x.out & 15)) return fail(D2D_ERR_PARAM, "pcm and out device pointers must be 16-byte aligned");
        if (blocks && (!x.pcm || !x.out)) return fail(D2D_ERR_PARAM, "pcm and out device pointers must be non-null");
        if (x.out_capacity_bytes < d2d_flac_bound_bytes(channels, bit_depth, x.frames, x.final)) return fail(D2D_ERR_CAPACITY, "out buffer below d2d_flac_bound_bytes");
        need += d2d_flac_workspace_bytes(channels, bit_depth, x.frames, x.final);
        any_blocks += blocks;
    }
    if (any_blocks && (!workspace || ((uintptr_t)workspace & 15))) return fail(D2D_ERR_PARAM, "workspace must be a 16-byte aligned device pointer");
    if (workspace_bytes < need) return fail(D2D_ERR_CAPACITY, "workspace below the sum of d2d_flac_workspace_bytes");

    hipStream_t s = (hipStream_t)hip_stream;
    const size_t slot = slot_bytes(channels, bit_depth);
    uint8_t* ws = (uint8_t*)workspace;
    for (uint32_t f0 = 0; f0 < n_files; f0 += MAXF) {
        const uint32_t nf = std::min<uint32_t>(MAXF, n_files - f0);
        FlacArgs a{};
        a.depth = bit_depth; a.slot_bytes = (uint32_t)slot;
        uint32_t max_blocks = 0;
        for (uint32_t i = 0; i < nf; ++i) {
            const d2d_flac_io& x = io[f0 + i];
            const size_t blocks = block_count(x.frames, x.final);
            FileDesc& d = a.f[i];
            d.pcm = (const uint8_t*)x.pcm; d.out = (uint8_t*)x.out; d.result = x.result;
            d.sizes = (uint32_t*)ws; d.slots = ws + align16(4 * blocks);
            d.blocks = (uint32_t)blocks; d.first_block = x.first_block;
            d.last_n = (x.final && x.frames % BS) ? (uint32_t)(x.frames % BS) : BS;
            ws += d2d_flac_workspace_bytes(channels, bit_depth, x.frames, x.final);
            max_blocks = std::max(max_blocks, d.blocks);
        }
        if (max_blocks) {
            hipError_t e = effort == D2D_FLAC_EFFORT_LPC ? launch_encode_ch<Encoder::search_lpc>(channels, a, max_blocks, nf, s)          // (the one place efforts become encoders)
                         : effort == D2D_FLAC_EFFORT_SEARCH ? launch_encode_ch<Encoder::search>(channels, a, max_blocks, nf, s) : launch_encode_ch<Encoder::fixed2>(channels, a, max_blocks, nf, s);
            if (e != hipSuccess) return hip_fail(e, effort == D2D_FLAC_EFFORT_FIXED2 ? "flac_encode_kernel" : "flac_search_kernel");
        }
        hipLaunchKernelGGL(flac_pack_kernel, dim3(std::max(1u, (max_blocks + PB - 1) / PB), nf), dim3(PT), 0, s, a);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return hip_fail(e, "flac_pack_kernel");
    }
    for (uint32_t f = 0; f < n_files; ++f) {
        io[f].blocks = block_count(io[f].frames, io[f].final);
        io[f].frames_consumed = io[f].final ? io[f].frames : (io[f].frames / BS) * BS;
    }
    return D2D_OK;
}

}  // extern "C"
