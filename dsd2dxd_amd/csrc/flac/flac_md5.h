// flac_md5.h -- STREAMINFO's MD5 (RFC 1321) of the unencoded audio as the host twin and the GPU kernel must agree on it bit for bit:
// the block function, the padding, and the rule that turns the packed PCM of the translate calls into the bytes FLAC hashes.  One copy,
// plain C++, compiled for the host (g++) and for the device (hipcc); no inline assembly -- the rotate and the selects are written in C
// and the compiler picks the instructions (v_alignbit_b32 for the rotate; what it does with the selects: DESIGN 4.6c).  (host/md5.h is
// the sink's and `verify`'s own MD5; tests hold the two to each other.)
//
// WHAT IS HASHED (FlacSink::write, host/pcm_sink.cpp): the interleaved samples as little-endian whole-byte integers.
//   16 and 24 bits: the packed frames as they are.
//   20 bits: the translate calls keep the value shifted left by 4 in a 3-byte container; FLAC hashes the 20-bit value itself, so every
//            3-byte sample is shifted right by 4 ARITHMETICALLY (the sign fills the top nibble) and emitted again as 3 bytes.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define D2D_MD5_HD __host__ __device__ __forceinline__
#else
#define D2D_MD5_HD inline
#endif

namespace d2dmd5 {

constexpr uint32_t BLOCK = 64;                                    // bytes of one MD5 block
constexpr uint32_t H0 = 0x67452301u, H1 = 0xefcdab89u, H2 = 0x98badcfeu, H3 = 0x10325476u;

D2D_MD5_HD uint32_t rol(uint32_t x, uint32_t s) { return (x << s) | (x >> (32 - s)); }
// the four round functions with one operation on the path from b, the value the previous step made:
// F and G are bit selects (b ? c : d, and d ? b : c), H leaves c ^ d off the chain, I leaves ~d off it
D2D_MD5_HD uint32_t f_sel(uint32_t b, uint32_t c, uint32_t d) { return d ^ (b & (c ^ d)); }
D2D_MD5_HD uint32_t g_sel(uint32_t b, uint32_t c, uint32_t d) { return c ^ (d & (b ^ c)); }
D2D_MD5_HD uint32_t h_xor(uint32_t b, uint32_t c, uint32_t d) { return b ^ (c ^ d); }
D2D_MD5_HD uint32_t i_orn(uint32_t b, uint32_t c, uint32_t d) { return c ^ (b | ~d); }

// one step: a = b + rol(a + f(b, c, d) + (K + m), s).  K + m and a + (K + m) do not depend on the step before: what waits for b is
// the select, one add, the rotate, one add.
#define D2D_MD5_STEP(f, a, b, c, d, mg, k, s) a = b + rol((a + ((k) + (mg))) + f(b, c, d), s)

// h += the compression of the 16 little-endian message words m
D2D_MD5_HD void block(uint32_t h[4], const uint32_t m[16]) {
    uint32_t a = h[0], b = h[1], c = h[2], d = h[3];
    D2D_MD5_STEP(f_sel, a, b, c, d, m[0], 0xd76aa478u, 7);   D2D_MD5_STEP(f_sel, d, a, b, c, m[1], 0xe8c7b756u, 12);
    D2D_MD5_STEP(f_sel, c, d, a, b, m[2], 0x242070dbu, 17);  D2D_MD5_STEP(f_sel, b, c, d, a, m[3], 0xc1bdceeeu, 22);
    D2D_MD5_STEP(f_sel, a, b, c, d, m[4], 0xf57c0fafu, 7);   D2D_MD5_STEP(f_sel, d, a, b, c, m[5], 0x4787c62au, 12);
    D2D_MD5_STEP(f_sel, c, d, a, b, m[6], 0xa8304613u, 17);  D2D_MD5_STEP(f_sel, b, c, d, a, m[7], 0xfd469501u, 22);
    D2D_MD5_STEP(f_sel, a, b, c, d, m[8], 0x698098d8u, 7);   D2D_MD5_STEP(f_sel, d, a, b, c, m[9], 0x8b44f7afu, 12);
    D2D_MD5_STEP(f_sel, c, d, a, b, m[10], 0xffff5bb1u, 17); D2D_MD5_STEP(f_sel, b, c, d, a, m[11], 0x895cd7beu, 22);
    D2D_MD5_STEP(f_sel, a, b, c, d, m[12], 0x6b901122u, 7);  D2D_MD5_STEP(f_sel, d, a, b, c, m[13], 0xfd987193u, 12);
    D2D_MD5_STEP(f_sel, c, d, a, b, m[14], 0xa679438eu, 17); D2D_MD5_STEP(f_sel, b, c, d, a, m[15], 0x49b40821u, 22);

    D2D_MD5_STEP(g_sel, a, b, c, d, m[1], 0xf61e2562u, 5);   D2D_MD5_STEP(g_sel, d, a, b, c, m[6], 0xc040b340u, 9);
    D2D_MD5_STEP(g_sel, c, d, a, b, m[11], 0x265e5a51u, 14); D2D_MD5_STEP(g_sel, b, c, d, a, m[0], 0xe9b6c7aau, 20);
    D2D_MD5_STEP(g_sel, a, b, c, d, m[5], 0xd62f105du, 5);   D2D_MD5_STEP(g_sel, d, a, b, c, m[10], 0x02441453u, 9);
    D2D_MD5_STEP(g_sel, c, d, a, b, m[15], 0xd8a1e681u, 14); D2D_MD5_STEP(g_sel, b, c, d, a, m[4], 0xe7d3fbc8u, 20);
    D2D_MD5_STEP(g_sel, a, b, c, d, m[9], 0x21e1cde6u, 5);   D2D_MD5_STEP(g_sel, d, a, b, c, m[14], 0xc33707d6u, 9);
    D2D_MD5_STEP(g_sel, c, d, a, b, m[3], 0xf4d50d87u, 14);  D2D_MD5_STEP(g_sel, b, c, d, a, m[8], 0x455a14edu, 20);
    D2D_MD5_STEP(g_sel, a, b, c, d, m[13], 0xa9e3e905u, 5);  D2D_MD5_STEP(g_sel, d, a, b, c, m[2], 0xfcefa3f8u, 9);
    D2D_MD5_STEP(g_sel, c, d, a, b, m[7], 0x676f02d9u, 14);  D2D_MD5_STEP(g_sel, b, c, d, a, m[12], 0x8d2a4c8au, 20);

    D2D_MD5_STEP(h_xor, a, b, c, d, m[5], 0xfffa3942u, 4);   D2D_MD5_STEP(h_xor, d, a, b, c, m[8], 0x8771f681u, 11);
    D2D_MD5_STEP(h_xor, c, d, a, b, m[11], 0x6d9d6122u, 16); D2D_MD5_STEP(h_xor, b, c, d, a, m[14], 0xfde5380cu, 23);
    D2D_MD5_STEP(h_xor, a, b, c, d, m[1], 0xa4beea44u, 4);   D2D_MD5_STEP(h_xor, d, a, b, c, m[4], 0x4bdecfa9u, 11);
    D2D_MD5_STEP(h_xor, c, d, a, b, m[7], 0xf6bb4b60u, 16);  D2D_MD5_STEP(h_xor, b, c, d, a, m[10], 0xbebfbc70u, 23);
    D2D_MD5_STEP(h_xor, a, b, c, d, m[13], 0x289b7ec6u, 4);  D2D_MD5_STEP(h_xor, d, a, b, c, m[0], 0xeaa127fau, 11);
    D2D_MD5_STEP(h_xor, c, d, a, b, m[3], 0xd4ef3085u, 16);  D2D_MD5_STEP(h_xor, b, c, d, a, m[6], 0x04881d05u, 23);
    D2D_MD5_STEP(h_xor, a, b, c, d, m[9], 0xd9d4d039u, 4);   D2D_MD5_STEP(h_xor, d, a, b, c, m[12], 0xe6db99e5u, 11);
    D2D_MD5_STEP(h_xor, c, d, a, b, m[15], 0x1fa27cf8u, 16); D2D_MD5_STEP(h_xor, b, c, d, a, m[2], 0xc4ac5665u, 23);

    D2D_MD5_STEP(i_orn, a, b, c, d, m[0], 0xf4292244u, 6);   D2D_MD5_STEP(i_orn, d, a, b, c, m[7], 0x432aff97u, 10);
    D2D_MD5_STEP(i_orn, c, d, a, b, m[14], 0xab9423a7u, 15); D2D_MD5_STEP(i_orn, b, c, d, a, m[5], 0xfc93a039u, 21);
    D2D_MD5_STEP(i_orn, a, b, c, d, m[12], 0x655b59c3u, 6);  D2D_MD5_STEP(i_orn, d, a, b, c, m[3], 0x8f0ccc92u, 10);
    D2D_MD5_STEP(i_orn, c, d, a, b, m[10], 0xffeff47du, 15); D2D_MD5_STEP(i_orn, b, c, d, a, m[1], 0x85845dd1u, 21);
    D2D_MD5_STEP(i_orn, a, b, c, d, m[8], 0x6fa87e4fu, 6);   D2D_MD5_STEP(i_orn, d, a, b, c, m[15], 0xfe2ce6e0u, 10);
    D2D_MD5_STEP(i_orn, c, d, a, b, m[6], 0xa3014314u, 15);  D2D_MD5_STEP(i_orn, b, c, d, a, m[13], 0x4e0811a1u, 21);
    D2D_MD5_STEP(i_orn, a, b, c, d, m[4], 0xf7537e82u, 6);   D2D_MD5_STEP(i_orn, d, a, b, c, m[11], 0xbd3af235u, 10);
    D2D_MD5_STEP(i_orn, c, d, a, b, m[2], 0x2ad7d2bbu, 15);  D2D_MD5_STEP(i_orn, b, c, d, a, m[9], 0xeb86d391u, 21);
    h[0] += a; h[1] += b; h[2] += c; h[3] += d;
}
#undef D2D_MD5_STEP

// the 20-bit rule on one sample: v holds the 3 container bytes (little-endian, bits 24 .. 31 ignored); the 3 bytes FLAC hashes
D2D_MD5_HD uint32_t sample20(uint32_t v) { return (uint32_t)((int32_t)(v << 8) >> 12) & 0xFFFFFFu; }

// message word i of a block from its bytes
D2D_MD5_HD uint32_t word_le(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }

// The digest of a message of `bytes` bytes whose whole blocks are in h and whose last bytes % 64 bytes are `tail`: the 0x80, the zeros
// and the 64-bit count of BITS, in one block, or in two where fewer than 8 bytes are left behind the 0x80.  Nothing it is given changes.
D2D_MD5_HD void finish(const uint32_t h_in[4], uint64_t bytes, const uint8_t* tail, uint8_t digest[16]) {
    uint32_t h[4] = {h_in[0], h_in[1], h_in[2], h_in[3]};
    const uint32_t t = (uint32_t)(bytes & 63u), wi = t >> 2, sh = 8 * (t & 3u);
    uint32_t m[16];
#if defined(__clang__)
    _Pragma("unroll")
#endif
    for (uint32_t i = 0; i < 16; ++i) {
        const uint32_t w = word_le(tail + 4 * i);
        m[i] = i < wi ? w : i == wi ? ((w & ((1u << sh) - 1u)) | (0x80u << sh)) : 0u;
    }
    if (t >= 56) {
        block(h, m);
#if defined(__clang__)
        _Pragma("unroll")
#endif
        for (uint32_t i = 0; i < 16; ++i) m[i] = 0;
    }
    const uint64_t bits = bytes << 3;                                 // mod 2^64, as RFC 1321 has it
    m[14] = (uint32_t)bits; m[15] = (uint32_t)(bits >> 32);
    block(h, m);
#if defined(__clang__)
    _Pragma("unroll")
#endif
    for (uint32_t i = 0; i < 16; ++i) digest[i] = (uint8_t)(h[i >> 2] >> (8 * (i & 3u)));
}

}  // namespace d2dmd5
