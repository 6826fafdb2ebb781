// flac_frame_enc.h -- the host FLAC frame encoder: the one copy that FlacSink (host/pcm_sink.cpp) and
// d2d_flac_encode_host (flac/d2d_flac_host.cpp) both run, and the byte-for-byte definition of what the GPU
// kernels of flac/d2d_flac.hip produce.  Host code only (no HIP).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

namespace d2dhost {

// FLAC with fixed-order-2 prediction and one Rice partition per subframe (valid, modest compression;
// the reference uses the flac-codec crate, Cargo.lock:299-307).  Integer depths only.  Frames are
// independent of each other, so a batch of them is encoded on as many threads and written in order.
struct FlacFrameEnc {
    std::vector<uint8_t> out;
    std::vector<int32_t> res;
    uint64_t bitacc = 0; int bitn = 0;
    // (the tables are function-local statics of class type: built once, by whichever thread asks first)
    struct Crc8Table { uint8_t t[256]; Crc8Table() { for (int i = 0; i < 256; ++i) { uint8_t c = (uint8_t)i; for (int k = 0; k < 8; ++k) c = (uint8_t)((c & 0x80) ? (c << 1) ^ 0x07 : (c << 1)); t[i] = c; } } };
    struct Crc16Table { uint16_t t[256]; Crc16Table() { for (int i = 0; i < 256; ++i) { uint16_t c = (uint16_t)(i << 8); for (int k = 0; k < 8; ++k) c = (uint16_t)((c & 0x8000) ? (c << 1) ^ 0x8005 : (c << 1)); t[i] = c; } } };
    static const uint8_t* crc8_table() { static const Crc8Table tab; return tab.t; }
    static const uint16_t* crc16_table() { static const Crc16Table tab; return tab.t; }
    static uint8_t crc8(const uint8_t* p, size_t n) { const uint8_t* t = crc8_table(); uint8_t c = 0; for (size_t i = 0; i < n; ++i) c = t[c ^ p[i]]; return c; }
    static uint16_t crc16(const uint8_t* p, size_t n) { const uint16_t* t = crc16_table(); uint16_t c = 0; for (size_t i = 0; i < n; ++i) c = (uint16_t)((c << 8) ^ t[(c >> 8) ^ p[i]]); return c; }
    void bits_put(uint64_t v, int n) {
        while (n > 0) {
            int take = n > 32 ? 32 : n;
            uint64_t part = (v >> (n - take)) & ((1ull << take) - 1);
            bitacc = (bitacc << take) | part; bitn += take; n -= take;
            while (bitn >= 8) { out.push_back((uint8_t)(bitacc >> (bitn - 8))); bitn -= 8; }
        }
    }
    void bits_flush() { if (bitn) { out.push_back((uint8_t)(bitacc << (8 - bitn))); bitn = 0; } bitacc = 0; }
    void put_utf8(uint32_t v) {
        if (v < 0x80) { bits_put(v, 8); return; }
        int n = v < 0x800 ? 1 : v < 0x10000 ? 2 : v < 0x200000 ? 3 : v < 0x4000000 ? 4 : 5;
        bits_put(((0xFF00 >> (n + 1)) & 0xFF) | (v >> (6 * n)), 8);
        for (int i = n - 1; i >= 0; --i) bits_put(0x80 | ((v >> (6 * i)) & 0x3F), 8);
    }
    // one frame of `n` interleaved samples starting at `buf`
    void encode(const int32_t* buf, uint32_t n, uint32_t ch, uint32_t depth, uint32_t frame_no, uint32_t BS) {
        out.clear(); bitn = 0; bitacc = 0;
        bits_put(0xFFF8, 16);                                          // sync, fixed block size
        bits_put(n == BS ? 0xC : 0x7, 4);                              // 4096, or 16-bit (n-1) at the end of the header
        bits_put(0x0, 4);                                              // sample rate from STREAMINFO
        bits_put(ch - 1, 4);                                           // independent channels
        bits_put(depth == 16 ? 4 : depth == 20 ? 5 : 6, 3); bits_put(0, 1);
        put_utf8(frame_no);
        if (n != BS) bits_put(n - 1, 16);
        bits_flush();
        out.push_back(crc8(out.data(), out.size()));
        res.resize(n);
        for (uint32_t c = 0; c < ch; ++c) {
            auto s = [&](uint32_t i) -> int64_t { return buf[(size_t)i * ch + c]; };
            const uint32_t order = n > 2 ? 2 : 0;
            uint64_t sum = 0;
            bool fits = true;
            for (uint32_t i = order; i < n; ++i) {
                int64_t r = order == 2 ? s(i) - 2 * s(i - 1) + s(i - 2) : s(i);
                if (r > 0x3FFFFFFF || r < -0x3FFFFFFF) fits = false;
                res[i] = (int32_t)r; sum += (uint64_t)(r < 0 ? -r : r);
            }
            if (!fits || order == 0) {                                   // verbatim subframe
                bits_put(0, 1); bits_put(1, 6); bits_put(0, 1);
                for (uint32_t i = 0; i < n; ++i) bits_put((uint64_t)s(i) & ((1ull << depth) - 1), (int)depth);
                continue;
            }
            bits_put(0, 1); bits_put(8 + order, 6); bits_put(0, 1);    // fixed predictor, no wasted bits
            for (uint32_t i = 0; i < order; ++i) bits_put((uint64_t)s(i) & ((1ull << depth) - 1), (int)depth);
            uint32_t k = 0;
            const uint64_t mean = sum / (n - order ? n - order : 1);
            while (k < 30 && (1ull << k) < mean) ++k;
            bits_put(1, 2);                                             // residual coding method 1: 5-bit Rice parameters
            bits_put(0, 4);                                             // partition order 0
            bits_put(k, 5);
            for (uint32_t i = order; i < n; ++i) {
                uint32_t u = res[i] >= 0 ? (uint32_t)res[i] << 1 : (((uint32_t)(-(int64_t)res[i])) << 1) - 1;
                uint32_t q = u >> k;
                while (q >= 32) { bits_put(0, 32); q -= 32; }
                bits_put(1, (int)q + 1);
                if (k) bits_put(u & ((1u << k) - 1), (int)k);
            }
        }
        bits_flush();
        uint16_t c16 = crc16(out.data(), out.size());
        out.push_back((uint8_t)(c16 >> 8)); out.push_back((uint8_t)c16);
    }
};

}  // namespace d2dhost
