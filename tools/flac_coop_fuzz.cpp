// flac_coop_fuzz.cpp -- the two verify methods (include/dsd2dxd_amd.h: D2D_FLAC_VERIFY_SERIAL, D2D_FLAC_VERIFY_COOP) on damaged frames,
// for a sanitizer build:
//   g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined -o flac_coop_fuzz \
//       tools/flac_coop_fuzz.cpp dsd2dxd_amd/csrc/flac/d2d_flac_host.cpp && ./flac_coop_fuzz SEED MUTATIONS
// CPU only (tests/test_flac_coop_cpu.py builds and runs it).  The cooperative rule (dsd2dxd_amd/csrc/flac/flac_expect.h) computes bit
// positions from the PCM and from fields of the frame and reads the frame there: on damaged frames those fields are anything.  Streams
// of three frames are encoded at every effort; each mutation damages the middle frame -- a bit flip, a byte splice, a truncation, a
// rewritten Rice parameter or partition order near the first subframe's head -- or the size table, and every other mutation has both
// CRCs repaired so that the rule's walk is reached.  The frames, the size table and the PCM lie in heap blocks of exactly their sizes:
// a read outside is a sanitizer report.  Both methods must give the same record, a block the fast path accepted must be good under the
// serial method, and the program prints how many blocks each path decided ("fast 6012", "fallback 3020") and "fuzz ok".
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../include/dsd2dxd_amd.h"

static uint64_t rng_state;
static uint32_t rng() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return (uint32_t)(rng_state >> 16); }

static uint8_t crc8(const uint8_t* p, size_t n) {
    uint32_t c = 0;
    for (size_t i = 0; i < n; ++i) { c ^= p[i]; for (int k = 0; k < 8; ++k) c = (c & 0x80u) ? ((c << 1) ^ 0x07u) & 0xFFu : (c << 1) & 0xFFu; }
    return (uint8_t)c;
}
static uint16_t crc16(const uint8_t* p, size_t n) {
    uint32_t c = 0;
    for (size_t i = 0; i < n; ++i) { c ^= (uint32_t)p[i] << 8; for (int k = 0; k < 8; ++k) c = (c & 0x8000u) ? ((c << 1) ^ 0x8005u) & 0xFFFFu : (c << 1) & 0xFFFFu; }
    return (uint16_t)c;
}

struct Stream {
    uint32_t channels, depth, effort, first_block;
    std::vector<uint32_t> ns;                  // samples per channel of each block
    std::vector<uint8_t> pcm;
    std::vector<std::vector<uint8_t>> frames;
    std::vector<uint32_t> header_bytes;
};

static void fail(const char* what) { printf("FAILED: %s (%s)\n", what, d2d_flac_error()); exit(1); }

static Stream make_stream(uint32_t channels, uint32_t depth, uint32_t effort, uint32_t first_block, uint32_t last_n) {
    Stream s{channels, depth, effort, first_block, {D2D_FLAC_BLOCK, D2D_FLAC_BLOCK, last_n}, {}, {}, {}};
    const uint32_t sb = depth == 16 ? 2 : 3;
    const size_t frames = 2 * (size_t)D2D_FLAC_BLOCK + last_n;
    s.pcm.resize(frames * channels * sb);
    const double top = (double)(1 << (depth - 2));
    for (size_t i = 0; i < frames; ++i)
        for (uint32_t c = 0; c < channels; ++c) {       // correlated channels, a tone and a little noise: stereo modes, LPC and fixed orders all win somewhere
            const double tone = top * sin(2 * M_PI * (300.0 + 900.0 * (double)(i / D2D_FLAC_BLOCK)) * (double)i / 88200.0 + 0.1 * c);
            int32_t v = (int32_t)lrint(tone * (c % 2 ? 0.8 : 1.0)) + (int32_t)(rng() % 33) - 16;
            if (depth == 20) v = (int32_t)((uint32_t)v << 4);
            uint8_t* q = &s.pcm[(i * channels + c) * sb];
            q[0] = (uint8_t)v; q[1] = (uint8_t)(v >> 8);
            if (sb == 3) q[2] = (uint8_t)(v >> 16);
        }
    size_t at = 0;
    for (size_t b = 0; b < s.ns.size(); ++b) {
        const uint32_t n = s.ns[b], number = first_block + (uint32_t)b;
        std::vector<uint8_t> out(d2d_flac_bound_bytes(channels, depth, n, 1));
        d2d_flac_result r;
        if (d2d_flac_encode_host_effort(channels, depth, effort, s.pcm.data() + at * channels * sb, n, number, 1, out.data(), out.size(), &r, nullptr) != D2D_OK) fail("encode");
        out.resize(r.bytes_out);
        s.frames.push_back(out);
        const uint32_t utf8 = number < 0x80 ? 1 : number < 0x800 ? 2 : number < 0x10000 ? 3 : number < 0x200000 ? 4 : number < 0x4000000 ? 5 : 6;
        s.header_bytes.push_back(4 + utf8 + (n != D2D_FLAC_BLOCK ? 2 : 0) + 1);
        at += n;
    }
    return s;
}

static unsigned long fast_total, fallback_total;

// both methods on one (possibly damaged) stream and size table, everything in exact heap blocks; returns the record
static d2d_flac_check run(const Stream& s, const std::vector<std::vector<uint8_t>>& frames, const std::vector<uint32_t>& table) {
    size_t total = 0, samples = 0;
    for (const auto& f : frames) total += f.size();
    for (uint32_t n : s.ns) samples += n;
    uint8_t* bytes = (uint8_t*)malloc(total ? total : 1);
    uint32_t* sizes = (uint32_t*)malloc(table.size() * sizeof(uint32_t));
    uint8_t* pcm = (uint8_t*)malloc(s.pcm.size());
    memcpy(pcm, s.pcm.data(), s.pcm.size());
    memcpy(sizes, table.data(), table.size() * sizeof(uint32_t));
    size_t at = 0;
    for (const auto& f : frames) { memcpy(bytes + at, f.data(), f.size()); at += f.size(); }
    d2d_flac_check serial, coop;
    d2d_flac_verify_stats st_serial, st_coop;
    if (d2d_flac_verify_host_method(s.channels, s.depth, pcm, samples, s.first_block, 1, bytes, total, sizes, &serial, D2D_FLAC_VERIFY_SERIAL, &st_serial) != D2D_OK) fail("serial");
    if (d2d_flac_verify_host_method(s.channels, s.depth, pcm, samples, s.first_block, 1, bytes, total, sizes, &coop, D2D_FLAC_VERIFY_COOP, &st_coop) != D2D_OK) fail("coop");
    if (memcmp(&serial, &coop, sizeof serial) != 0) {
        printf("serial: %llu %u %u %u %u; coop: %llu %u %u %u %u\n", (unsigned long long)serial.samples_checked, serial.blocks_checked, serial.bad_blocks, serial.first_bad_block,
               serial.first_bad_reason, (unsigned long long)coop.samples_checked, coop.blocks_checked, coop.bad_blocks, coop.first_bad_block, coop.first_bad_reason);
        fail("the two methods give different records");
    }
    if (st_serial.fast_blocks != 0 || st_serial.fallback_blocks != serial.blocks_checked) fail("the serial method's stats");
    if (st_coop.fast_blocks + st_coop.fallback_blocks != coop.blocks_checked) fail("the cooperative method's stats do not add up");
    if (st_coop.fast_blocks > serial.blocks_checked - serial.bad_blocks) fail("the fast path accepted a block the serial parser calls bad");
    fast_total += st_coop.fast_blocks; fallback_total += st_coop.fallback_blocks;
    free(pcm); free(sizes); free(bytes);
    return serial;
}

static std::vector<uint32_t> table_of(const std::vector<std::vector<uint8_t>>& frames) {
    std::vector<uint32_t> t;
    for (const auto& f : frames) t.push_back((uint32_t)f.size());
    return t;
}

// `width` bits at bit `pos` of f, most significant first
static void set_bits(std::vector<uint8_t>& f, size_t pos, uint32_t width, uint32_t value) {
    for (uint32_t i = 0; i < width; ++i, ++pos) {
        if (pos / 8 >= f.size()) return;
        const uint8_t m = (uint8_t)(0x80u >> (pos % 8));
        f[pos / 8] = (uint8_t)(((value >> (width - 1 - i)) & 1u) ? f[pos / 8] | m : f[pos / 8] & ~m);
    }
}

int main(int argc, char** argv) {
    rng_state = (argc > 1 ? strtoull(argv[1], 0, 10) : 1) * 0x9E3779B97F4A7C15ull + 0xD1B54A32D192ED03ull;
    const int mutations = argc > 2 ? atoi(argv[2]) : 3000;
    std::vector<Stream> streams;
    const uint32_t efforts[3] = {D2D_FLAC_EFFORT_FIXED2, D2D_FLAC_EFFORT_SEARCH, D2D_FLAC_EFFORT_LPC};
    for (uint32_t e : efforts) {
        streams.push_back(make_stream(2, 24, e, 0, 100));
        streams.push_back(make_stream(1, 16, e, 126, 2));
        streams.push_back(make_stream(3, 20, e, 0xFFFE, 1000));
    }
    for (const Stream& s : streams) {
        const d2d_flac_check c = run(s, s.frames, table_of(s.frames));
        if (c.bad_blocks || c.first_bad_block != 0xFFFFFFFFu || c.blocks_checked != 3) fail("an undamaged stream did not verify");
    }
    if (fast_total != 3 * streams.size() || fallback_total != 0) fail("the fast path did not accept every undamaged block");
    for (int m = 0; m < mutations; ++m) {
        const Stream& s = streams[rng() % streams.size()];
        std::vector<std::vector<uint8_t>> frames = s.frames;
        std::vector<uint8_t>& f = frames[1];
        const uint32_t hb = s.header_bytes[1], size = (uint32_t)f.size();
        auto offset = [&]() -> uint32_t {                           // the offset classes
            switch (rng() % 4) {
                case 0: return rng() % hb;                          // the header
                case 1: return hb + rng() % 2;                      // the first subframe's head
                case 2: return rng() % size;                        // anywhere
                default: return size - 1 - rng() % 5;               // the last code, the padding, the CRC-16
            }
        };
        bool table_too = true;
        switch (rng() % 6) {
            case 0: f[offset()] ^= (uint8_t)(1u << (rng() % 8)); break;
            case 1: {                                               // a splice: bytes from elsewhere in the frame
                const uint32_t to = offset(), len = 1 + rng() % 8, from = rng() % size;
                for (uint32_t i = 0; i < len && to + i < size && from + i < size; ++i) f[to + i] = s.frames[1][from + i];
                break;
            }
            case 2: f.resize(offset()); break;                      // a truncation (down to nothing), the table following it
            case 3: f.resize(offset()); table_too = false; break;   // ... or not: the table then reaches beyond the bytes
            case 4: set_bits(f, 8 * hb + rng() % (40 + 3 * s.depth), 5, rng() % 32); break;      // a 5-bit field near the head: parameters, orders, shifts
            default: f[hb] = (uint8_t)(rng() % 256); break;         // the subframe's type
        }
        if (m % 2) {                                                // repair both CRCs
            if (f.size() >= hb) f[hb - 1] = crc8(f.data(), hb - 1);
            if (f.size() >= 2) { const uint16_t c = crc16(f.data(), f.size() - 2); f[f.size() - 2] = (uint8_t)(c >> 8); f[f.size() - 1] = (uint8_t)c; }
        }
        std::vector<uint32_t> table = table_too ? table_of(frames) : table_of(s.frames);
        if (rng() % 8 == 0) table[rng() % 3] += (rng() % 2 ? 1u : 0u - 1u) * (1 + rng() % 3);      // a wrong size entry
        if (rng() % 32 == 0) table[rng() % 3] = rng();
        const d2d_flac_check c = run(s, frames, table);
        if (c.blocks_checked != 3 || c.first_bad_reason > D2D_FLAC_BAD_SAMPLES) fail("not a record");
    }
    printf("mutations %d\nfast %lu\nfallback %lu\n", mutations, fast_total, fallback_total);
    printf("fuzz ok\n");
    return 0;
}
