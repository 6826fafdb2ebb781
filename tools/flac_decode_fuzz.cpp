// flac_decode_fuzz.cpp -- the FLAC frame parser (dsd2dxd_amd/csrc/flac/flac_parse.h) and the host readers built on it
// (d2d_flac_host.cpp: d2d_flac_verify_host, d2d_flac_decode_host) on damaged frames, for a sanitizer build:
//   g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined -o flac_decode_fuzz \
//       tools/flac_decode_fuzz.cpp dsd2dxd_amd/csrc/flac/d2d_flac_host.cpp && ./flac_decode_fuzz SEED MUTATIONS
// CPU only (tests/test_flac_verify_cpu.py builds and runs it).  Streams of three frames are encoded at every effort; each mutation
// damages the middle frame -- a bit flip, a byte splice or a truncation, at an offset in the header, at the first subframe's head,
// anywhere, or in the last bytes -- and every other mutation has both CRCs repaired, so that the parser behind them is reached.  The
// frames, the size table and the PCM lie in heap blocks of exactly their sizes: a read outside the frame is a sanitizer report.  Every
// outcome must be a reason: the program prints how many mutations reached each ("reached SAMPLES 412") and "fuzz ok" at the end.
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

// the three readers on one (possibly damaged) stream, everything in exact heap blocks; returns the size-table verifier's record
static d2d_flac_check run(const Stream& s, const std::vector<std::vector<uint8_t>>& frames) {
    size_t total = 0, samples = 0;
    for (const auto& f : frames) total += f.size();
    for (uint32_t n : s.ns) samples += n;
    uint8_t* bytes = (uint8_t*)malloc(total ? total : 1);
    uint32_t* sizes = (uint32_t*)malloc(frames.size() * sizeof(uint32_t));
    uint8_t* pcm = (uint8_t*)malloc(s.pcm.size());
    memcpy(pcm, s.pcm.data(), s.pcm.size());
    size_t at = 0;
    for (size_t b = 0; b < frames.size(); ++b) { memcpy(bytes + at, frames[b].data(), frames[b].size()); at += frames[b].size(); sizes[b] = (uint32_t)frames[b].size(); }
    d2d_flac_check with_sizes, walked, decoded;
    if (d2d_flac_verify_host(s.channels, s.depth, pcm, samples, s.first_block, 1, bytes, total, sizes, &with_sizes) != D2D_OK) fail("verify with sizes");
    if (d2d_flac_verify_host(s.channels, s.depth, pcm, samples, s.first_block, 1, bytes, total, nullptr, &walked) != D2D_OK) fail("verify walking");
    uint8_t* back = (uint8_t*)malloc(s.pcm.size());
    size_t frames_out = 0;
    const int rc = d2d_flac_decode_host(s.channels, s.depth, bytes, total, s.first_block, back, s.pcm.size(), &frames_out, &decoded);
    if (rc != D2D_OK && rc != D2D_ERR_CAPACITY) fail("decode");        // (a damaged header may announce more samples than the stream held)
    if (rc == D2D_OK && decoded.bad_blocks == 0) {
        // what decodes cleanly and is not the PCM must have been caught by the verifier (20-bit: the container's low nibble is not coded)
        bool same = frames_out == samples;
        for (size_t i = 0; same && i < s.pcm.size(); ++i) same = s.depth == 20 && i % 3 == 0 ? (back[i] & 0xF0) == (pcm[i] & 0xF0) : back[i] == pcm[i];
        if (same != (with_sizes.bad_blocks == 0)) fail("the decoder and the verifier disagree");
    }
    if ((with_sizes.bad_blocks == 0) != (walked.bad_blocks == 0) && with_sizes.first_bad_reason != D2D_FLAC_BAD_LENGTH && with_sizes.first_bad_reason != D2D_FLAC_BAD_SIZE)
        fail("the two verifiers disagree on whether the stream is good");
    free(back); free(pcm); free(sizes); free(bytes);
    return with_sizes;
}

int main(int argc, char** argv) {
    rng_state = (argc > 1 ? strtoull(argv[1], 0, 10) : 1) * 0x9E3779B97F4A7C15ull + 0xD1B54A32D192ED03ull;
    const int mutations = argc > 2 ? atoi(argv[2]) : 2000;
    static const char* const names[] = {"NONE", "SIZE", "HEADER", "CRC8", "CRC16", "UNSUPPORTED", "SYNTAX", "LENGTH", "SAMPLES"};
    std::vector<Stream> streams;
    const uint32_t efforts[3] = {D2D_FLAC_EFFORT_FIXED2, D2D_FLAC_EFFORT_SEARCH, D2D_FLAC_EFFORT_LPC};
    for (uint32_t e : efforts) {
        streams.push_back(make_stream(2, 24, e, 0, 100));
        streams.push_back(make_stream(1, 16, e, 126, 2));
        streams.push_back(make_stream(3, 20, e, 0xFFFE, 1000));
    }
    for (const Stream& s : streams) {
        const d2d_flac_check c = run(s, s.frames);
        if (c.bad_blocks || c.first_bad_block != 0xFFFFFFFFu || c.blocks_checked != 3) fail("an undamaged stream did not verify");
    }
    unsigned long reached[9] = {};
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
        switch (rng() % 3) {
            case 0: f[offset()] ^= (uint8_t)(1u << (rng() % 8)); break;
            case 1: {                                               // a splice: bytes from elsewhere in the frame
                const uint32_t to = offset(), len = 1 + rng() % 8, from = rng() % size;
                for (uint32_t i = 0; i < len && to + i < size && from + i < size; ++i) f[to + i] = s.frames[1][from + i];
                break;
            }
            default: f.resize(offset()); break;                     // a truncation (down to nothing)
        }
        if (m % 2) {                                                // repair both CRCs
            if (f.size() >= hb) f[hb - 1] = crc8(f.data(), hb - 1);
            if (f.size() >= 2) { const uint16_t c = crc16(f.data(), f.size() - 2); f[f.size() - 2] = (uint8_t)(c >> 8); f[f.size() - 1] = (uint8_t)c; }
        }
        const d2d_flac_check c = run(s, frames);
        if (c.blocks_checked != 3 || c.first_bad_reason > D2D_FLAC_BAD_SAMPLES) fail("not a record");
        if (c.bad_blocks && c.first_bad_block == 0) fail("the undamaged first block was blamed");
        ++reached[c.first_bad_reason];
    }
    for (int r = 0; r < 9; ++r) printf("reached %s %lu\n", names[r], reached[r]);
    printf("fuzz ok\n");
    return 0;
}
