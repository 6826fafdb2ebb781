// d2d_flac.hip -- FLAC frames on the GPU (gfx950): the kernels behind d2d_flac_encode_device, and d2d_convert_stream_flac on top
// of the public calls.  The bitstream is the one flac_frame_enc.h defines, at every effort; tests/test_gpu_flac.py (effort 0),
// tests/test_gpu_flac_search.py (effort 1) and tests/test_gpu_flac_lpc.py (effort 12) compare them byte for byte.
//
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
#include "flac_lpc.h"

using namespace d2dflac;

namespace {

constexpr int NT = 1024;          // threads of an encode workgroup
constexpr int NW = NT / 64;
constexpr int SPT = BS / NT;      // samples per thread and channel
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

// `len` (1..32) bits of `val` at bit `pos` of the image, most significant bit first
__device__ __forceinline__ void put_bits(uint32_t* img, uint32_t pos, uint32_t val, uint32_t len) {
    const uint32_t w = pos >> 5, o = pos & 31;
    const uint64_t v = (uint64_t)val << (64 - o - len);
    const uint32_t hi = (uint32_t)(v >> 32), lo = (uint32_t)v;
    if (hi) atomicOr(&img[w], hi);
    if (lo) atomicOr(&img[w + 1], lo);
}

// a * b in GF(2)[x] / (x^16 + x^15 + x^2 + 1)
__device__ __forceinline__ uint32_t gf_mul(uint32_t a, uint32_t b) {
    uint32_t r = 0;
    for (int i = 15; i >= 0; --i) {
        r <<= 1;
        if (r & 0x10000u) r ^= 0x18005u;
        if ((b >> i) & 1u) r ^= a;
    }
    return r;
}
__device__ __forceinline__ uint32_t gf_xpow(uint32_t e) {     // x^e
    uint32_t r = 1, base = 2;
    for (; e; e >>= 1) { if (e & 1u) r = gf_mul(r, base); base = gf_mul(base, base); }
    return r;
}

// the CRC-16 table (x^16 + x^15 + x^2 + 1)
__device__ __forceinline__ void build_crc_tab(uint16_t* s_crc_tab, uint32_t tid) {
    if (tid < 256) {
        uint32_t c = tid << 8;
        for (int i = 0; i < 8; ++i) c = (c & 0x8000u) ? ((c << 1) ^ 0x8005u) & 0xFFFFu : (c << 1) & 0xFFFFu;
        s_crc_tab[tid] = (uint16_t)c;
    }
}

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

// CRC-16 of the image's first data_bytes, placed behind them.  The whole workgroup, all bits of the image placed and a barrier passed;
// ends with a barrier.
__device__ __forceinline__ void frame_crc16(uint32_t* img, uint32_t data_bytes, const uint16_t* s_crc_tab, uint16_t* s_crc, uint32_t tid) {
    auto image_byte = [&](uint32_t j) -> uint32_t { return (img[j >> 2] >> (24 - 8 * (j & 3))) & 0xFFu; };
    const uint32_t L = (data_bytes + NT - 1) / NT, padz = NT * L - data_bytes;
    uint32_t c = 0;
    for (uint32_t v = tid * L; v < (tid + 1) * L; ++v)
        if (v >= padz) c = ((c << 8) & 0xFFFFu) ^ s_crc_tab[(c >> 8) ^ image_byte(v - padz)];
    s_crc[tid] = (uint16_t)c;
    uint32_t m = gf_xpow(8 * L);
    for (uint32_t stride = 1; stride < NT; stride <<= 1) {
        __syncthreads();
        if ((tid & (2 * stride - 1)) == 0) s_crc[tid] = (uint16_t)(gf_mul(s_crc[tid], m) ^ s_crc[tid + stride]);
        m = gf_mul(m, m);
    }
    __syncthreads();
    if (tid == 0 && s_crc[0]) put_bits(img, data_bytes * 8, s_crc[0], 16);
    __syncthreads();
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

template <int CH>
__global__ __launch_bounds__(NT) void flac_encode_kernel(const FlacArgs a) {
    extern __shared__ __align__(16) unsigned char smem[];          // the block's PCM, then the frame image
    __shared__ unsigned long long s_wsum[NW][CH];
    __shared__ uint32_t s_wtot[NW][CH];
    __shared__ uint32_t s_k[CH];
    __shared__ uint16_t s_crc_tab[256];
    __shared__ uint16_t s_crc[NT];
    __shared__ uint8_t s_hdr[16];

    const FileDesc& fd = a.f[blockIdx.y];
    const uint32_t b = blockIdx.x;
    if (b >= fd.blocks) return;                                     // (the whole workgroup)
    const uint32_t n = b + 1 == fd.blocks ? fd.last_n : BS;
    const uint32_t depth = a.depth, sb = depth == 16 ? 2u : 3u, fb = CH * sb;
    const uint32_t order = n > 2 ? 2u : 0u;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t frame_no = fd.first_block + b;
    const uint32_t hdr_bytes = 4 + utf8_len(frame_no) + (n != BS ? 2u : 0u) + 1;

    // 1. PCM -> LDS
    {
        const uint8_t* src = fd.pcm + (size_t)b * BS * fb;
        const uint32_t nbytes = n * fb, nvec = nbytes >> 4;
        for (uint32_t v = tid; v < nvec; v += NT) reinterpret_cast<uint4*>(smem)[v] = reinterpret_cast<const uint4*>(src)[v];
        for (uint32_t j = (nvec << 4) + tid; j < nbytes; j += NT) smem[j] = src[j];
    }
    build_crc_tab(s_crc_tab, tid);
    if (tid == 0) build_header(s_hdr, n, CH - 1, depth, frame_no);
    __syncthreads();

    // 2. samples -> residuals (warm-up and verbatim samples stay as they are), sum |r|
    int32_t val[CH][SPT];
    const uint32_t i0 = tid * SPT;
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
            if (i < n && i >= order && order == 2) {                // |r| <= 2^25: the sink's verbatim escape (30 bits) cannot fire
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
    if (lane == 0) {
#pragma unroll
        for (int c = 0; c < CH; ++c) s_wsum[wave][c] = asum[c];
    }
    __syncthreads();
    if (tid < CH) {
        unsigned long long sum = 0;
        for (int w = 0; w < NW; ++w) sum += s_wsum[w][tid];
        const unsigned long long mean = sum / (n > 2 ? n - 2 : 1);
        uint32_t k = 0;
        while (k < 30 && (1ull << k) < mean) ++k;
        s_k[tid] = k;
    }
    __syncthreads();

    // 3. code lengths and where every thread's bits begin
    uint32_t kk[CH], start[CH];
    uint32_t total_bits = hdr_bytes * 8;
    {
        uint32_t incl[CH], mine[CH];
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            const uint32_t k = s_k[c];
            kk[c] = k;
            uint32_t len = tid == 0 ? 8 + (order == 2 ? 11u : 0u) : 0;          // subframe header; residual header in front of sample 2
#pragma unroll
            for (int j = 0; j < SPT; ++j) {
                const uint32_t i = i0 + j;
                if (i >= n) continue;
                if (i < 2 || order == 0) len += depth;
                else {
                    const int32_t r = val[c][j];
                    const uint32_t u = r >= 0 ? (uint32_t)r << 1 : ((uint32_t)(-r) << 1) - 1;
                    len += (u >> k) + 1 + k;
                }
            }
            mine[c] = len;
            uint32_t x = len;
            for (int o = 1; o < 64; o <<= 1) { const uint32_t y = __shfl_up(x, o, 64); if (lane >= (uint32_t)o) x += y; }
            incl[c] = x;
        }
        if (lane == 63) {
#pragma unroll
            for (int c = 0; c < CH; ++c) s_wtot[wave][c] = incl[c];
        }
        __syncthreads();
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            uint32_t before = 0, all = 0;
            for (int w = 0; w < NW; ++w) { const uint32_t t = s_wtot[w][c]; all += t; if ((uint32_t)w < wave) before += t; }
            start[c] = total_bits + before + incl[c] - mine[c];
            total_bits += all;
        }
    }
    const uint32_t data_bytes = (total_bits + 7) >> 3, frame_bytes = data_bytes + 2;
    const uint32_t out_vecs = (frame_bytes + 15) >> 4;
    // (frame_bytes <= slot_bytes by the bound of include/dsd2dxd_amd.h; a frame that broke it would be dropped whole, not written past the image)
    if (frame_bytes > a.slot_bytes) { if (tid == 0) fd.sizes[b] = 0; return; }

    // 4. the image: zero fill, then the bits that are one
    uint32_t* img = reinterpret_cast<uint32_t*>(smem);
    for (uint32_t w = tid; w < out_vecs * 4 + 4; w += NT) img[w] = 0;             // (every thread has passed the barriers behind its PCM reads)
    __syncthreads();
    if (tid < hdr_bytes && s_hdr[tid]) put_bits(img, tid * 8, s_hdr[tid], 8);
#pragma unroll
    for (int c = 0; c < CH; ++c) {
        uint32_t p = start[c];
        const uint32_t k = kk[c];
        if (tid == 0) { put_bits(img, p, order == 2 ? 0x14u : 0x02u, 8); p += 8; }   // 0 001010 0: fixed order 2; 0 000001 0: verbatim
#pragma unroll
        for (int j = 0; j < SPT; ++j) {
            const uint32_t i = i0 + j;
            if (i >= n) continue;
            if (i == 2 && order == 2) { put_bits(img, p, (1u << 9) | k, 11); p += 11; }   // 01: 5-bit Rice parameters, 0000: one partition, k
            if (i < 2 || order == 0) {
                const uint32_t raw = (uint32_t)val[c][j] & ((1u << depth) - 1);
                if (raw) put_bits(img, p, raw, depth);
                p += depth;
            } else {
                const int32_t r = val[c][j];
                const uint32_t u = r >= 0 ? (uint32_t)r << 1 : ((uint32_t)(-r) << 1) - 1;
                const uint32_t q = u >> k;
                put_bits(img, p + q, (1u << k) | (u & ((1u << k) - 1)), k + 1);
                p += q + 1 + k;
            }
        }
    }
    __syncthreads();

    // 5. CRC-16 over the data_bytes in front of it; 6. image -> slot
    frame_crc16(img, data_bytes, s_crc_tab, s_crc, tid);
    store_frame(img, fd.slots + (size_t)b * a.slot_bytes, out_vecs, tid);
    if (tid == 0) fd.sizes[b] = frame_bytes;
}

// ---- effort 1: the search of flac_frame_enc.h -------------------------------------------------------------------------------

constexpr int NP = 64;            // Rice partitions of a whole block at the finest partition order, 6: 64 samples, 16 lanes each

__device__ __forceinline__ uint32_t zigzag(int32_t r) { return r >= 0 ? (uint32_t)r << 1 : ((uint32_t)(-r) << 1) - 1; }
__device__ __forceinline__ uint32_t rice_k(unsigned long long sum, uint32_t count) {
    const unsigned long long mean = sum / (count ? count : 1);
    uint32_t k = 0;
    while (k < 30 && (1ull << k) < mean) ++k;
    return k;
}
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
// Sums across lanes without LDS traffic: four DPP adds leave the sum of each row of 16 lanes in all its lanes (lane ^ 1, lane ^ 2 by
// quad permutes, then the half row and the row mirrored); four lane reads add the rows of a wave into a wave-uniform value.  Every
// lane of the wave must be active.
template <int CTRL>
__device__ __forceinline__ uint32_t dpp_move(uint32_t v) { return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xF, 0xF, true); }
__device__ __forceinline__ uint32_t row_sum(uint32_t v) {
    v += dpp_move<0xB1>(v);                                          // quad_perm [1, 0, 3, 2]
    v += dpp_move<0x4E>(v);                                          // quad_perm [2, 3, 0, 1]
    v += dpp_move<0x141>(v);                                         // row_half_mirror
    v += dpp_move<0x140>(v);                                         // row_mirror
    return v;
}
__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
    v = row_sum(v);
    return (uint32_t)(__builtin_amdgcn_readlane((int)v, 0) + __builtin_amdgcn_readlane((int)v, 16) + __builtin_amdgcn_readlane((int)v, 32) +
                      __builtin_amdgcn_readlane((int)v, 48));
}
// ... of 64-bit values below 2^48 as two 32-bit sums of 24-bit halves: neither can overflow over 64 lanes
__device__ __forceinline__ unsigned long long row_sum(unsigned long long v) {
    return ((unsigned long long)row_sum((uint32_t)(v >> 24)) << 24) + row_sum((uint32_t)v & 0xFFFFFFu);
}
__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
    return ((unsigned long long)wave_sum((uint32_t)(v >> 24)) << 24) + wave_sum((uint32_t)v & 0xFFFFFFu);
}
// v[i] summed over the workgroup, in every thread; N sums share the two barriers.  32-bit sums must fit 32 bits, 64-bit sums 48.
template <int N, typename T>
__device__ __forceinline__ void wg_sum(T (&v)[N], unsigned long long* s_red, uint32_t lane, uint32_t wave) {
    T* red = reinterpret_cast<T*>(s_red);
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] = wave_sum(v[i]);
    __syncthreads();                                                 // (the readers of the last use are through)
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < N; ++i) red[wave * N + i] = v[i];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] = row_sum(red[(lane & (NW - 1)) * N + i]);      // 16 lanes hold the 16 waves' sums
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

//   flac_search_kernel<CH, LPC>   the same workgroup, with the decisions of effort 1 between "PCM in LDS" and "place bits".  Candidate
//   signals (the channels; for two channels also mid and side) go through (a) to (c) one at a time, so that one signal's five
//   residual sets are all the registers hold:
//     (a) sum |r_o| for o = 0 .. 4, one five-wide 64-bit reduction; threads 0 .. 4 derive the five k; the code lengths under them,
//         one five-wide reduction; every thread picks the order from the five exact costs
//     (b) sum |r| of the chosen order per finest partition (n >> pmax samples): for a whole block 16 lanes, one DPP row sum; for
//         a short block whatever the samples fall into, by LDS adds.  Threads 0 .. 126 add them up to the partitions of every order
//         p <= pmax and derive their k: the table s_kt
//     (c) every thread's code lengths under each p's k, one seven-wide reduction; every thread picks the partition order; the chosen
//         order's k row is kept per signal
//     (d) two channels: the assignment from the four signals' costs
//     (e) per subframe the chosen signal's residuals again, now kept; lengths with the residual header in front of sample `order` and
//         a 5-bit k in front of every partition's first residual; then the scan, the image, the CRC and the slot as at effort 0.
//   A frame of fewer than 16 samples takes the same path with the choices forced to effort 0's.
//   LPC (effort 12, rules 9 to 19 of flac_frame_enc.h; frames of 64 samples and more): behind (c) a signal goes through
//     (f) y = the windowed signal into an LDS plane of its own behind the PCM; every thread's part of R(0 .. 12) from its four y and
//         their twelve predecessors, 64-bit; three-limb wave sums, then 64-bit LDS adds: exact, whatever the order of arrival
//     (g) thread 0 runs flac_lpc.h from R to the quantised coefficients of orders 4, 8 and 12; the others wait at the barrier
//     (h) the three residual sets by 64-bit multiply-adds from the PCM plane, their k and their costs at one partition as in (a)
//     (i) (b) and (c) once more for the best order; the signal keeps its effort-1 plan unless this one is strictly cheaper
//   and (e) forms an LPC subframe's residuals and header from the kept coefficients.
template <int CH, bool LPC>
__global__ __launch_bounds__(NT) void flac_search_kernel(const FlacArgs a) {
    constexpr int NSIG = CH == 2 ? 4 : CH;
    extern __shared__ __align__(16) unsigned char smem[];          // the block's PCM as planar 32-bit samples, then the frame image
    __shared__ unsigned long long s_red[NW * 8];
    __shared__ unsigned long long s_psum[NP];
    __shared__ uint32_t s_wtot[NW][CH];
    __shared__ uint32_t s_ko[5];
    __shared__ uint32_t s_sel[NSIG][3];                             // order, partition order, cost of each signal
    __shared__ uint8_t s_kt[2 * NP];                                // k of partition j at partition order p: s_kt[2^p - 1 + j]
    __shared__ uint8_t s_ksel[NSIG][NP];                            // ... the chosen order's row
    __shared__ unsigned long long s_R[LPC ? d2dlpc::MAX_ORDER + 1 : 1];
    __shared__ int32_t s_co[LPC ? d2dlpc::CANDIDATES * d2dlpc::MAX_ORDER + d2dlpc::CANDIDATES + 1 : 1];   // q, the shifts, the valid bits
    __shared__ int32_t s_lq[LPC ? NSIG : 1][d2dlpc::MAX_ORDER + 2];  // a signal's kept coefficients (zero from its order on), shift, and whether its plan is LPC
    __shared__ uint16_t s_crc_tab[256];
    __shared__ uint16_t s_crc[NT];
    __shared__ uint8_t s_hdr[16];

    const FileDesc& fd = a.f[blockIdx.y];
    const uint32_t b = blockIdx.x;
    if (b >= fd.blocks) return;                                     // (the whole workgroup)
    const uint32_t n = b + 1 == fd.blocks ? fd.last_n : BS;
    const uint32_t depth = a.depth, sb = depth == 16 ? 2u : 3u, fb = CH * sb;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t frame_no = fd.first_block + b;
    const uint32_t hdr_bytes = 4 + utf8_len(frame_no) + (n != BS ? 2u : 0u) + 1;
    const bool searched = n >= 16;
    // the largest p <= 6 with n % 2^p == 0 and (n >> p) >= 16; the finest partitions and where this thread's samples lie in them
    const uint32_t pmax = searched ? min(6u, min((uint32_t)__ffs(n) - 1u, 27u - (uint32_t)__clz(n))) : 0u;
    const uint32_t fsz = n >> pmax, i0 = tid * SPT, pj0 = i0 / fsz, rem0 = i0 - pj0 * fsz;

    int32_t* pcm = reinterpret_cast<int32_t*>(smem);
    int32_t* yplane = pcm + CH * BS;                                // (LPC only: the launch asks for it)
    load_planar<CH>(pcm, fd.pcm + (size_t)b * BS * fb, n, depth, tid);
    build_crc_tab(s_crc_tab, tid);
    __syncthreads();

#pragma unroll 1
    for (uint32_t sg = 0; sg < (uint32_t)NSIG; ++sg) {
        const uint32_t bits = CH == 2 && sg == 3 ? depth + 1 : depth;
        if (tid < NP) s_psum[tid] = 0;                              // (read last before the barriers of the previous round's sums)
        // (a) the five residual sets as u = zigzag(r); |r| = (u + 1) >> 1
        uint32_t u[5][SPT];
        unsigned long long asum[5];
        {
            int32_t x[8];
            load_window<CH>(x, pcm, i0, n, sg);
#pragma unroll
            for (int o = 0; o < 5; ++o) {
                if (o) difference(x, o);
                uint32_t acc = 0;                                   // |r_4| <= 2^28: four of them fit
#pragma unroll
                for (int j = 0; j < SPT; ++j) {
                    u[o][j] = zigzag(x[4 + j]);
                    if (i0 + j < n && i0 + j >= (uint32_t)o) acc += (u[o][j] + 1) >> 1;
                }
                asum[o] = acc;
            }
        }
        wg_sum<5>(asum, s_red, lane, wave);
        if (tid < 5) s_ko[tid] = rice_k(tid == 0 ? asum[0] : tid == 1 ? asum[1] : tid == 2 ? asum[2] : tid == 3 ? asum[3] : asum[4], n > tid ? n - tid : 1);
        __syncthreads();
        uint32_t len[5];
#pragma unroll
        for (int o = 0; o < 5; ++o) {
            const uint32_t k = s_ko[o];
            len[o] = 0;
#pragma unroll
            for (int j = 0; j < SPT; ++j)
                if (i0 + j < n && i0 + j >= (uint32_t)o) len[o] += (u[o][j] >> k) + 1 + k;
        }
        wg_sum<5>(len, s_red, lane, wave);
        uint32_t order = 0, cost = 0;
#pragma unroll
        for (int o = 0; o < 5; ++o) {                               // the smallest order wins a tie
            const uint32_t c = 8 + o * bits + 6 + 5 + len[o];
            if (o == 0 || c < cost) { order = o; cost = c; }
        }
        if (!searched) order = n > 2 ? 2u : n;                      // effort 0's frame: order 2, or verbatim (every sample a warm-up)

        uint32_t uo[SPT];
#pragma unroll
        for (int j = 0; j < SPT; ++j) uo[j] = order == 0 ? u[0][j] : order == 1 ? u[1][j] : order == 2 ? u[2][j] : order == 3 ? u[3][j] : u[4][j];
        uint32_t hdrbits = 8 + order * bits + 6;                    // in front of the partitions: subframe header, warm-up, 01 pppp
        uint32_t cost1 = 0, lbest = 0;
        // pass 0: (b) and (c) for the fixed order; LPC only, pass 1: (f) to (h), then (b) and (c) again for the best LPC order.
        // (The loop's body keeps effort 1's indentation: with LPC = false it is effort 1's code, run once.)
#pragma unroll 1
        for (int pass = 0; pass < (LPC ? 2 : 1); ++pass) {
        if (LPC && pass == 1) {
            if (n < d2dlpc::MIN_FRAME) break;
            if (tid < NP) s_psum[tid] = 0;                          // (read last before the barriers of pass 0's sums)
            // (f) the windowed signal, its autocorrelation
            {
                int32_t xw[16];
                load_window16<CH>(xw, pcm, i0, n, sg);
                const uint32_t ws = d2dlpc::lpc_window_shift(n);
                int32_t y[SPT];
#pragma unroll
                for (int j = 0; j < SPT; ++j) y[j] = i0 + j < n ? d2dlpc::lpc_window(xw[12 + j], i0 + j, n, ws) : 0;
                *reinterpret_cast<int4*>(yplane + i0) = make_int4(y[0], y[1], y[2], y[3]);
            }
            if (tid <= (uint32_t)d2dlpc::MAX_ORDER) s_R[tid] = 0;
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
                for (int l = 0; l <= d2dlpc::MAX_ORDER; ++l) {
                    long long part = 0;                             // |y| <= 2^24: a thread's part stays below 2^50, a wave's below 2^56
#pragma unroll
                    for (int j = 0; j < SPT; ++j) part += (long long)yw[12 + j] * yw[12 + j - l];
                    part = wave_sum_i64(part);
                    if (lane == 0) atomicAdd(&s_R[l], (unsigned long long)part);
                }
            }
            __syncthreads();
            // (g) from R to coefficients: one lane
            if (tid == 0) {
                int64_t R[d2dlpc::MAX_ORDER + 1];
#pragma unroll
                for (int l = 0; l <= d2dlpc::MAX_ORDER; ++l) R[l] = (int64_t)s_R[l];
                d2dlpc::LpcCoefs co;
                d2dlpc::lpc_coefficients(R, co);
#pragma unroll
                for (int c = 0; c < d2dlpc::CANDIDATES; ++c) {
                    if (!(co.valid >> c & 1u)) continue;
#pragma unroll
                    for (int j = 0; j < d2dlpc::MAX_ORDER; ++j) s_co[c * d2dlpc::MAX_ORDER + j] = j < 4 * (c + 1) ? co.q[c][j] : 0;
                    s_co[d2dlpc::CANDIDATES * d2dlpc::MAX_ORDER + c] = co.shift[c];
                }
                s_co[d2dlpc::CANDIDATES * (d2dlpc::MAX_ORDER + 1)] = (int32_t)co.valid;
            }
            __syncthreads();
            const uint32_t valid = (uint32_t)s_co[d2dlpc::CANDIDATES * (d2dlpc::MAX_ORDER + 1)];
            if (!valid) break;
            // (h) the residuals of the three orders, their costs at one partition
            int32_t xw[16];
            load_window16<CH>(xw, pcm, i0, n, sg);
            uint32_t ul[d2dlpc::CANDIDATES][SPT];
            unsigned long long lsum[d2dlpc::CANDIDATES];
#pragma unroll
            for (int c = 0; c < d2dlpc::CANDIDATES; ++c) {
                unsigned long long acc = 0;                         // |r| < 2^30
                if (valid >> c & 1u) {
                    int32_t r[SPT];
                    lpc_residuals4(r, xw, &s_co[c * d2dlpc::MAX_ORDER], s_co[d2dlpc::CANDIDATES * d2dlpc::MAX_ORDER + c]);
#pragma unroll
                    for (int j = 0; j < SPT; ++j) {
                        ul[c][j] = zigzag(r[j]);
                        if (i0 + j < n && i0 + j >= 4u * (c + 1)) acc += (ul[c][j] + 1) >> 1;
                    }
                } else {
#pragma unroll
                    for (int j = 0; j < SPT; ++j) ul[c][j] = 0;
                }
                lsum[c] = acc;
            }
            wg_sum<d2dlpc::CANDIDATES>(lsum, s_red, lane, wave);
            if (tid < (uint32_t)d2dlpc::CANDIDATES) s_ko[tid] = rice_k(tid == 0 ? lsum[0] : tid == 1 ? lsum[1] : lsum[2], n - 4 * (tid + 1));
            __syncthreads();
            uint32_t llen[d2dlpc::CANDIDATES];
#pragma unroll
            for (int c = 0; c < d2dlpc::CANDIDATES; ++c) {
                const uint32_t k = s_ko[c];
                llen[c] = 0;
#pragma unroll
                for (int j = 0; j < SPT; ++j)
                    if (i0 + j < n && i0 + j >= 4u * (c + 1)) llen[c] += (ul[c][j] >> k) + 1 + k;
            }
            wg_sum<d2dlpc::CANDIDATES>(llen, s_red, lane, wave);
            bool any = false;
            uint32_t lcost = 0;
#pragma unroll
            for (int c = 0; c < d2dlpc::CANDIDATES; ++c) {         // the smaller order wins a tie
                const uint32_t P = 4 * (c + 1), cc = 8 + P * bits + 9 + 14 * P + 6 + 5 + llen[c];
                if ((valid >> c & 1u) && (!any || cc < lcost)) { any = true; lbest = c; lcost = cc; }
            }
            order = 4 * (lbest + 1);
            hdrbits = 8 + order * bits + 9 + 14 * order + 6;
#pragma unroll
            for (int j = 0; j < SPT; ++j) uo[j] = lbest == 0 ? ul[0][j] : lbest == 1 ? ul[1][j] : ul[2][j];
        }

        // (b) sum |r| per finest partition, then k for every partition of every order
        if (n == BS) {                                              // 16 lanes hold one partition
            unsigned long long t = 0;
#pragma unroll
            for (int j = 0; j < SPT; ++j) if (i0 + j >= order) t += (uo[j] + 1) >> 1;
            t = row_sum(t);
            if ((lane & 15u) == 0) s_psum[tid >> 4] = t;
        } else {
            unsigned long long run = 0;
            uint32_t pj = pj0, rem = rem0;
#pragma unroll
            for (int j = 0; j < SPT; ++j) {
                if (i0 + j < n && i0 + j >= order) run += (uo[j] + 1) >> 1;
                const bool ends = j == SPT - 1 || rem + 1 == fsz;
                if (ends && run) { atomicAdd(&s_psum[pj], run); run = 0; }     // (run != 0 only below n: pj < 2^pmax)
                if (++rem == fsz) { rem = 0; ++pj; }
            }
        }
        __syncthreads();
        if (tid < 2 * NP - 1) {
            const uint32_t p = 31u - (uint32_t)__clz(tid + 1), j = tid + 1 - (1u << p);
            if (p <= pmax) {
                const uint32_t span = 1u << (pmax - p);
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
        {
            uint32_t pj = pj0, rem = rem0;
#pragma unroll
            for (int j = 0; j < SPT; ++j) {
                if (i0 + j < n && i0 + j >= order) {
#pragma unroll
                    for (int p = 0; p < 7; ++p)
                        if ((uint32_t)p <= pmax) { const uint32_t k = s_kt[(1u << p) - 1 + (pj >> (pmax - p))]; plen[p] += (uo[j] >> k) + 1 + k; }
                }
                if (++rem == fsz) { rem = 0; ++pj; }
            }
        }
        wg_sum<7>(plen, s_red, lane, wave);
        uint32_t porder = 0;
#pragma unroll
        for (int p = 0; p < 7; ++p) {                               // the smallest partition order wins a tie
            const uint32_t c = hdrbits + (5u << p) + plen[p];
            if (p == 0) cost = c;
            else if ((uint32_t)p <= pmax && c < cost) { porder = p; cost = c; }
        }
        if (LPC && pass == 1) {                                     // (i) the LPC plan only where it is strictly cheaper
            if (!(cost < cost1)) break;
            if (tid < (uint32_t)d2dlpc::MAX_ORDER) s_lq[sg][tid] = s_co[lbest * d2dlpc::MAX_ORDER + tid];
            if (tid == 0) { s_lq[sg][d2dlpc::MAX_ORDER] = s_co[d2dlpc::CANDIDATES * d2dlpc::MAX_ORDER + lbest]; s_lq[sg][d2dlpc::MAX_ORDER + 1] = 1; }
        } else if (LPC && tid == 0) s_lq[sg][d2dlpc::MAX_ORDER + 1] = 0;
        cost1 = cost;
        if (tid == 0) { s_sel[sg][0] = order; s_sel[sg][1] = porder; s_sel[sg][2] = cost; }
        if (tid < (1u << porder)) s_ksel[sg][tid] = s_kt[(1u << porder) - 1 + tid];
        }
    }
    __syncthreads();

    // (d) the channel assignment: independent, left/side, side/right, mid/side; ties in this order
    uint32_t mode = 0;
    if (CH == 2 && searched) {
        const uint32_t L = s_sel[0][2], R = s_sel[1][2], M = s_sel[NSIG > 2 ? 2 : 0][2], S = s_sel[NSIG > 3 ? 3 : 0][2];
        uint32_t total = L + R;
        if (L + S < total) { total = L + S; mode = 1; }
        if (S + R < total) { total = S + R; mode = 2; }
        if (M + S < total) { total = M + S; mode = 3; }
    }
    if (tid == 0) build_header(s_hdr, n, mode == 0 ? CH - 1 : 7 + mode, depth, frame_no);
    auto subframe_signal = [&](int c) -> uint32_t {
        if (CH != 2) return (uint32_t)c;
        return c == 0 ? (mode == 2 ? 3u : mode == 3 ? 2u : 0u) : (mode == 0 || mode == 2 ? 1u : 3u);
    };

    // (e) the chosen residuals (warm-up samples as they are), code lengths, and where every thread's bits begin
    int32_t val[CH][SPT];
    uint32_t start[CH];
    uint32_t total_bits = hdr_bytes * 8;
    {
        uint32_t incl[CH], mine[CH];
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            const uint32_t sg = subframe_signal(c), order = s_sel[sg][0], sh = pmax - s_sel[sg][1];
            const uint32_t bits = CH == 2 && sg == 3 ? depth + 1 : depth;
            int32_t x[8];
            int32_t raw[SPT];
            const bool lp = LPC && s_lq[LPC ? sg : 0][d2dlpc::MAX_ORDER + 1];
            if (LPC && lp) {
                int32_t xw[16], r[SPT];
                load_window16<CH>(xw, pcm, i0, n, sg);
                lpc_residuals4(r, xw, s_lq[sg], s_lq[sg][d2dlpc::MAX_ORDER]);
#pragma unroll
                for (int j = 0; j < SPT; ++j) { raw[j] = xw[12 + j]; x[4 + j] = r[j]; }
            } else {
            load_window<CH>(x, pcm, i0, n, sg);
#pragma unroll
            for (int j = 0; j < SPT; ++j) raw[j] = x[4 + j];
#pragma unroll
            for (int o = 1; o < 5; ++o) if ((uint32_t)o <= order) difference(x, o);
            }
            uint32_t len = tid == 0 ? 8 : 0;                        // the subframe header
            uint32_t pj = pj0, rem = rem0;
#pragma unroll
            for (int j = 0; j < SPT; ++j) {
                const uint32_t i = i0 + j;
                val[c][j] = i < order ? raw[j] : x[4 + j];
                if (i < n) {
                    if (i < order) len += bits;
                    else {
                        if (i == order) len += 6;                   // 01 pppp
                        if (LPC && lp && i == order) len += 9 + 14 * order;     // 1101 sssss and the coefficients
                        if (i == order || (rem == 0 && (pj & ((1u << sh) - 1)) == 0)) len += 5;     // a partition's first residual: kkkkk
                        const uint32_t k = s_ksel[sg][pj >> sh];
                        len += (zigzag(val[c][j]) >> k) + 1 + k;
                    }
                }
                if (++rem == fsz) { rem = 0; ++pj; }
            }
            mine[c] = len;
            uint32_t y = len;
            for (int o = 1; o < 64; o <<= 1) { const uint32_t z = __shfl_up(y, o, 64); if (lane >= (uint32_t)o) y += z; }
            incl[c] = y;
        }
        if (lane == 63) {
#pragma unroll
            for (int c = 0; c < CH; ++c) s_wtot[wave][c] = incl[c];
        }
        __syncthreads();
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            uint32_t all = s_wtot[lane & (NW - 1)][c], before = (lane & (NW - 1)) < wave ? all : 0;      // 16 lanes hold the 16 waves' totals
            for (int o = NW / 2; o >= 1; o >>= 1) { all += __shfl_xor(all, o, 64); before += __shfl_xor(before, o, 64); }
            start[c] = total_bits + before + incl[c] - mine[c];
            total_bits += all;
        }
    }
    const uint32_t data_bytes = (total_bits + 7) >> 3, frame_bytes = data_bytes + 2;
    const uint32_t out_vecs = (frame_bytes + 15) >> 4;
    // (an effort-1 frame is no longer than the effort-0 frame, so the bound of include/dsd2dxd_amd.h holds; as there, a frame that broke it would be dropped whole)
    if (frame_bytes > a.slot_bytes) { if (tid == 0) fd.sizes[b] = 0; return; }

    // the image: zero fill, then the bits that are one
    uint32_t* img = reinterpret_cast<uint32_t*>(smem);
    for (uint32_t w = tid; w < out_vecs * 4 + 4; w += NT) img[w] = 0;             // (every thread has passed the barrier behind its PCM reads)
    __syncthreads();
    if (tid < hdr_bytes && s_hdr[tid]) put_bits(img, tid * 8, s_hdr[tid], 8);
#pragma unroll
    for (int c = 0; c < CH; ++c) {
        const uint32_t sg = subframe_signal(c), order = s_sel[sg][0], porder = s_sel[sg][1], sh = pmax - porder;
        const uint32_t bits = CH == 2 && sg == 3 ? depth + 1 : depth;
        uint32_t p = start[c];
        const bool lp = LPC && s_lq[LPC ? sg : 0][d2dlpc::MAX_ORDER + 1];
        if (LPC && lp) { if (tid == 0) { put_bits(img, p, (0x20u | (order - 1)) << 1, 8); p += 8; } }   // 0 1ppppp 0: LPC order ppppp + 1
        else
        if (tid == 0) { put_bits(img, p, n > 2 ? (8u | order) << 1 : 0x02u, 8); p += 8; }   // 0 001ooo 0: fixed order ooo; 0 000001 0: verbatim
        uint32_t pj = pj0, rem = rem0;
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
                        put_bits(img, p, ((uint32_t)(d2dlpc::PRECISION - 1) << 5) | (uint32_t)s_lq[sg][d2dlpc::MAX_ORDER], 9); p += 9;
                        for (uint32_t m = 0; m < order; ++m) { put_bits(img, p, (uint32_t)s_lq[sg][m] & 0x3FFFu, d2dlpc::PRECISION); p += d2dlpc::PRECISION; }
                    }
                    if (i == order) { put_bits(img, p, (1u << 4) | porder, 6); p += 6; }          // 01: 5-bit Rice parameters, pppp
                    if (i == order || (rem == 0 && (pj & ((1u << sh) - 1)) == 0)) { if (k) put_bits(img, p, k, 5); p += 5; }
                    const uint32_t v = zigzag(val[c][j]), q = v >> k;
                    put_bits(img, p + q, (1u << k) | (v & ((1u << k) - 1)), k + 1);
                    p += q + 1 + k;
                }
            }
            if (++rem == fsz) { rem = 0; ++pj; }
        }
    }
    __syncthreads();

    frame_crc16(img, data_bytes, s_crc_tab, s_crc, tid);
    store_frame(img, fd.slots + (size_t)b * a.slot_bytes, out_vecs, tid);
    if (tid == 0) fd.sizes[b] = frame_bytes;
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

// the frame image over the block's PCM: packed as it comes at effort 0, planar 32-bit samples in the search kernel, whose LPC flavour
// (`effort` 2 here) keeps the windowed signal's plane behind them
size_t encode_lds_bytes(uint32_t ch, uint32_t depth, int effort) {
    return std::max<size_t>(slot_bytes(ch, depth) + 32, (size_t)BS * ch * (effort ? 4 : sample_bytes(depth)) + (effort == 2 ? (size_t)BS * 4 : 0));
}

template <int CH, int EFFORT>
hipError_t launch_encode(const FlacArgs& a, uint32_t max_blocks, uint32_t nf, hipStream_t s) {
    const auto kernel = EFFORT == 0 ? &flac_encode_kernel<CH> : EFFORT == 1 ? &flac_search_kernel<CH, false> : &flac_search_kernel<CH, true>;
    // hipFuncSetAttribute acts on the current device: remembered per device, under a lock
    static std::mutex mu;
    static size_t allowed[64] = {};
    const size_t lds = encode_lds_bytes(CH, a.depth, EFFORT);
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

template <int EFFORT>
hipError_t launch_encode_ch(uint32_t ch, const FlacArgs& a, uint32_t max_blocks, uint32_t nf, hipStream_t s) {
    switch (ch) {
        case 1: return launch_encode<1, EFFORT>(a, max_blocks, nf, s);
        case 2: return launch_encode<2, EFFORT>(a, max_blocks, nf, s);
        case 3: return launch_encode<3, EFFORT>(a, max_blocks, nf, s);
        case 4: return launch_encode<4, EFFORT>(a, max_blocks, nf, s);
        case 5: return launch_encode<5, EFFORT>(a, max_blocks, nf, s);
        case 6: return launch_encode<6, EFFORT>(a, max_blocks, nf, s);
        case 7: return launch_encode<7, EFFORT>(a, max_blocks, nf, s);
        default: return launch_encode<8, EFFORT>(a, max_blocks, nf, s);
    }
}

int hip_fail(hipError_t e, const char* what) { return fail(D2D_ERR_DEVICE, std::string(what) + ": " + hipGetErrorString(e)); }

}  // namespace

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
            hipError_t e = effort == D2D_FLAC_EFFORT_LPC ? launch_encode_ch<2>(channels, a, max_blocks, nf, s)
                         : effort == D2D_FLAC_EFFORT_SEARCH ? launch_encode_ch<1>(channels, a, max_blocks, nf, s) : launch_encode_ch<0>(channels, a, max_blocks, nf, s);
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

// ---- the whole-stream driver ---------------------------------------------------------------------------------------------------

namespace {

struct DevBuf {
    void* p = nullptr; size_t bytes = 0;
    ~DevBuf() { if (p) (void)hipFree(p); }
    hipError_t alloc(size_t n) { bytes = n; return hipMalloc(&p, std::max<size_t>(n, 16)); }
};
struct PinBuf {
    void* p = nullptr;
    ~PinBuf() { if (p) (void)hipHostFree(p); }
    hipError_t alloc(size_t n) { return hipHostMalloc(&p, std::max<size_t>(n, 16), hipHostMallocDefault); }
};
// All device work of the stream driver goes to the null stream: the engine remembers the stream of its last call (d2d_peak waits on
// it), so it must not be one that ends with this function.  (The buffers' release waits for the device.)
struct Stream { hipStream_t s = nullptr; };

}  // namespace

#define FLAC_HIP(call, what) do { hipError_t e_ = (call); if (e_ != hipSuccess) return hip_fail(e_, what); } while (0)

extern "C" int d2d_convert_stream_flac(d2d_engine* e, uint32_t bit_depth, d2d_read_fn read, void* ru, d2d_write_fn write, void* wu,
                                       const volatile int* cancel, d2d_progress_fn progress, void* pu,
                                       uint64_t total, size_t chunk, d2d_flac_stream_stats* stats) {
    return d2d_convert_stream_flac_effort(e, bit_depth, D2D_FLAC_EFFORT_FIXED2, read, ru, write, wu, cancel, progress, pu, total, chunk, stats);
}

extern "C" int d2d_convert_stream_flac_effort(d2d_engine* e, uint32_t bit_depth, uint32_t effort, d2d_read_fn read, void* ru,
                                              d2d_write_fn write, void* wu, const volatile int* cancel, d2d_progress_fn progress, void* pu,
                                              uint64_t total, size_t chunk, d2d_flac_stream_stats* stats) {
    if (!effort_ok(effort)) return fail(D2D_ERR_PARAM, EFFORT_MESSAGE);
    if (!e) return fail(D2D_ERR_PARAM, "null engine");
    if (!read) return fail(D2D_ERR_PARAM, "null read callback");
    if (!stats) return fail(D2D_ERR_PARAM, "null stats");
    if (!depth_ok(bit_depth)) return fail(D2D_ERR_PARAM, "FLAC holds 16, 20 or 24-bit integers (Invalid bit depth)");
    const size_t fb = d2d_frame_bytes(e), sb = sample_bytes(bit_depth);
    if (fb == 0 || fb % sb || fb / sb > 8) return fail(D2D_ERR_PARAM, "the engine's frames do not hold 1 to 8 channels of this bit depth");
    const uint32_t ch = (uint32_t)(fb / sb);
    if (chunk == 0) chunk = 1u << 22;
    // the engine's device becomes this thread's current device (d2d_peak selects it and waits for the engine's pending work)
    double peak0 = 0.0;
    if (d2d_peak(e, 0, 0, &peak0) != D2D_OK) return fail(D2D_ERR_DEVICE, d2d_last_error(e));
    *stats = d2d_flac_stream_stats{0, 0, 0, 0};

    // frames one chunk can add: the engine's own count for a chunk from where it stands, and a margin for the rounding of later ones
    const size_t chunk_frames = d2d_next_frames(e, 0, chunk) + 64, cap_frames = chunk_frames + BS;
    const size_t out_cap = d2d_flac_bound_bytes(ch, bit_depth, cap_frames, 1), ws_cap = d2d_flac_workspace_bytes(ch, bit_depth, cap_frames, 1);
    Stream st;
    PinBuf h_in[2], h_out, h_res;
    DevBuf d_in, d_new, d_pcm, d_out, d_ws;
    FLAC_HIP(h_in[0].alloc(chunk * ch), "hipHostMalloc"); FLAC_HIP(h_in[1].alloc(chunk * ch), "hipHostMalloc");
    FLAC_HIP(h_out.alloc(out_cap), "hipHostMalloc"); FLAC_HIP(h_res.alloc(sizeof(d2d_flac_result)), "hipHostMalloc");
    FLAC_HIP(d_in.alloc(chunk * ch), "hipMalloc"); FLAC_HIP(d_new.alloc(chunk_frames * fb), "hipMalloc");
    FLAC_HIP(d_pcm.alloc(cap_frames * fb), "hipMalloc"); FLAC_HIP(d_out.alloc(out_cap), "hipMalloc"); FLAC_HIP(d_ws.alloc(ws_cap), "hipMalloc");
    d2d_flac_result* res = (d2d_flac_result*)h_res.p;

    size_t carry = 0;                 // frames in front of d_pcm that no block has taken yet
    uint64_t done = 0;
    int cur = 0;
    long got = read(ru, (uint8_t*)h_in[cur].p, chunk);
    if (got < 0) return fail(D2D_ERR_IO, "read callback failed");
    while (got > 0) {
        if (cancel && *cancel) return fail(D2D_ERR_CANCELLED, "Conversion cancelled");
        const size_t L = (size_t)got;
        if (L > chunk) return fail(D2D_ERR_IO, "read callback returned more than it was asked for");
        // upload and convert; the PCM lands in a buffer of its own (the translate call wants 16-byte alignment, the end of the carry
        // has none) and is copied behind the carry on the same stream
        d2d_file_io tio{};
        tio.dsd = d_in.p; tio.bytes_per_channel = L; tio.pcm = d_new.p; tio.pcm_capacity_bytes = d_new.bytes;
        FLAC_HIP(hipMemcpyAsync(d_in.p, h_in[cur].p, L * ch, hipMemcpyHostToDevice, st.s), "hipMemcpyAsync");
        if (d2d_translate_batch_device(e, &tio, 1, st.s) != D2D_OK) return fail(D2D_ERR_DEVICE, d2d_last_error(e));
        const size_t nf = tio.frames_out;
        if (carry + nf > cap_frames) return fail(D2D_ERR_STATE, "a chunk produced more frames than planned");
        if (nf) FLAC_HIP(hipMemcpyAsync((uint8_t*)d_pcm.p + carry * fb, d_new.p, nf * fb, hipMemcpyDeviceToDevice, st.s), "hipMemcpyAsync");
        // the next chunk is read while the GPU works: the stream ends with this chunk if there is none
        const long next = read(ru, (uint8_t*)h_in[cur ^ 1].p, chunk);
        if (next < 0) return fail(D2D_ERR_IO, "read callback failed");
        d2d_flac_io fio{};
        fio.pcm = d_pcm.p; fio.frames = carry + nf; fio.first_block = (uint32_t)stats->blocks; fio.final = next == 0;
        fio.out = d_out.p; fio.out_capacity_bytes = d_out.bytes; fio.result = res;
        if (stats->blocks > 0xFFFFFFFFull) return fail(D2D_ERR_PARAM, "frame numbers are 31 bits");
        const int rc = d2d_flac_encode_device_effort(ch, bit_depth, effort, &fio, 1, d_ws.p, d_ws.bytes, st.s);
        if (rc != D2D_OK) return rc;
        FLAC_HIP(hipStreamSynchronize(st.s), "hipStreamSynchronize");
        const d2d_flac_result r = *res;
        if (r.bytes_out) {
            FLAC_HIP(hipMemcpy(h_out.p, d_out.p, r.bytes_out, hipMemcpyDeviceToHost), "hipMemcpy");
            if (write && write(wu, h_out.p, r.bytes_out) != 0) return fail(D2D_ERR_IO, "write callback failed");
        }
        if (fio.blocks) {
            stats->min_frame_bytes = stats->blocks ? std::min(stats->min_frame_bytes, r.min_frame_bytes) : r.min_frame_bytes;
            stats->max_frame_bytes = std::max(stats->max_frame_bytes, r.max_frame_bytes);
            stats->blocks += fio.blocks;
            stats->samples_per_channel += fio.frames_consumed;
        }
        // the remainder moves to the front (it lies wholly behind its destination: a block was taken, or nothing moves)
        carry = fio.frames - fio.frames_consumed;
        if (carry && fio.frames_consumed)
            FLAC_HIP(hipMemcpyAsync(d_pcm.p, (uint8_t*)d_pcm.p + fio.frames_consumed * fb, carry * fb, hipMemcpyDeviceToDevice, st.s), "hipMemcpyAsync");
        done += (uint64_t)L;
        if (progress && total) {
            float pct = (float)(100.0 * (double)done / (double)total);
            if (pct >= 100.0f) pct = 99.99f;       // exactly 100 is reserved for the end
            progress(pu, pct);
        }
        got = next; cur ^= 1;
    }
    if (progress) progress(pu, 100.0f);
    return D2D_OK;
}
