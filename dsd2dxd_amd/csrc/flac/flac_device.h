// flac_device.h -- the device helpers the FLAC kernels share: the encode kernels (d2d_flac.hip) and the cooperative verify kernel
// (d2d_flac_verify.hip) both run one workgroup of NT threads per (file, block), thread t owning samples 4t .. 4t+3 of every channel, and
// both need bits placed in an LDS image, the parallel CRC-16 over that image, the scan that turns code lengths into bit positions, and
// sums across lanes.  One copy, here.  Device code only (hipcc).
#pragma once
#include <hip/hip_runtime.h>

#include "d2d_flac_internal.h"

namespace d2dflac {

constexpr int NT = 1024;          // threads of an encode workgroup
constexpr int NW = NT / 64;
constexpr int SPT = BS / NT;      // samples per thread and channel

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

// What a workgroup knows of its block before it reads a sample.  Passed by value: every field is uniform or a function of the thread.
struct Block {
    uint32_t n, depth;                              // samples per channel, their bits
    uint32_t tid, lane, wave, i0;                   // this thread; its first sample
    uint32_t frame_no, hdr_bytes;
    uint32_t pmax, fsz, pj0, rem0;                  // the search: rule 6's pmax; a finest partition's samples, n >> pmax; i0 = pj0 * fsz + rem0
};

// Step 3: where this thread's bits of every channel begin, from its code lengths mine[c]: an inclusive scan over the wave's lanes, the
// 16 waves' totals through LDS into 16 lanes; channel 0 starts at first_bit.  Returns the bits behind the last channel.  One barrier.
template <int CH>
__device__ __forceinline__ uint32_t scan_starts(uint32_t (&start)[CH], const uint32_t (&mine)[CH], uint32_t first_bit, uint32_t (*s_wtot)[CH], const Block B) {
    uint32_t incl[CH];
#pragma unroll
    for (int c = 0; c < CH; ++c) {
        uint32_t x = mine[c];
        for (int o = 1; o < 64; o <<= 1) { const uint32_t y = __shfl_up(x, o, 64); if (B.lane >= (uint32_t)o) x += y; }
        incl[c] = x;
    }
    if (B.lane == 63) {
#pragma unroll
        for (int c = 0; c < CH; ++c) s_wtot[B.wave][c] = incl[c];
    }
    __syncthreads();
    uint32_t total_bits = first_bit;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
        uint32_t all = s_wtot[B.lane & (NW - 1)][c], before = (B.lane & (NW - 1)) < B.wave ? all : 0;
        for (int o = NW / 2; o >= 1; o >>= 1) { all += __shfl_xor(all, o, 64); before += __shfl_xor(before, o, 64); }
        start[c] = total_bits + before + incl[c] - mine[c];
        total_bits += all;
    }
    return total_bits;
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

}  // namespace d2dflac
