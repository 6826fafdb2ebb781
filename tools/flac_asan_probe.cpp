// flac_asan_probe.cpp -- the host FLAC encoder (dsd2dxd_amd/csrc/flac/d2d_flac_host.cpp: d2d_flac_encode_host_effort, i.e. the sink's
// FlacFrameEnc) at every effort on the adversarial signals of tests/flac_ref.py, in heap buffers of exactly the declared sizes, for a
// sanitizer build:
//   g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -o flac_asan_probe \
//       tools/flac_asan_probe.cpp dsd2dxd_amd/csrc/flac/d2d_flac_host.cpp && ./flac_asan_probe
// CPU only; prints one line per (channels, depth) and effort with the bytes produced and an FNV-1a of them, and "ok" at the end.
// Effort 1 also runs the lengths at which the search changes its partition range (16, 17, 32, 1024) and must never produce more bytes
// than effort 0; effort 12 runs every length, those around its shortest LPC frame (63, 64, 65) among them, on a sixth signal as well --
// coloured noise, what LPC predictors are there for -- and must never produce more bytes than effort 1.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../include/dsd2dxd_amd.h"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull, extra_state = 0xD1B54A32D192ED03ull, lpc_state = 0xA0761D6478BD642Full;
static uint32_t rng() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return (uint32_t)(rng_state >> 16); }

static int32_t sample(int sig, size_t i, uint32_t c, size_t frames, uint32_t depth) {
    const int32_t hi = (1 << (depth - 1)) - 1, lo = -(1 << (depth - 1));
    switch (sig) {
        case 0: return 0;                                                  // digital silence
        case 1: return (i + c) % 2 ? lo : hi;                              // alternating full scale
        case 2: return i == (frames / 2 + 37 * c) % frames ? (c % 2 ? lo : hi) : 0;      // one spike in silence
        case 3: return (int32_t)(rng() % (uint32_t)(hi - lo + 1)) + lo;    // uniform random
        case 4: return (int32_t)lrint(hi * sin(2 * M_PI * 1000.0 * (double)i / 88200.0 + 0.7 * c));
        default: return 0;                                                 // (coloured noise has state: see coloured())
    }
}

// noise through two resonant pole pairs, an eighth of full scale: one value per call, in the order the samples are drawn
static double col_y[8][4];
static int32_t coloured(uint32_t c, uint32_t depth) {
    static const double a[4] = {-2.3, 2.8498, -1.98927, 0.74805};         // (1 - 1.6 z^-1 + r^2 z^-2)(1 - 0.7 z^-1 + r^2 z^-2), r = 0.93
    double v = ((double)(rng() & 0xFFFF) - 32768.0) / 32768.0 * (double)(1 << (depth - 8));
    for (int j = 0; j < 4; ++j) v -= a[j] * col_y[c][j];
    for (int j = 3; j > 0; --j) col_y[c][j] = col_y[c][j - 1];
    col_y[c][0] = v;
    const double top = (double)((1 << (depth - 1)) - 1);
    return (int32_t)lrint(v > top ? top : v < -top ? -top : v);
}

int main() {
    const size_t lengths[] = {2 * 4096 + 1000, 4096, 4097, 4098, 4099, 4095, 1, 2, 3, 0, 16, 17, 32, 1024, 63, 64, 65};
    const size_t n_effort1 = 14;                                               // effort 1 runs the first fourteen, as it always has
    const uint32_t efforts[3] = {D2D_FLAC_EFFORT_FIXED2, D2D_FLAC_EFFORT_SEARCH, D2D_FLAC_EFFORT_LPC};
    const size_t n_effort0 = 10;                                               // effort 0 runs the first ten, as it always has
    for (uint32_t ch : {1u, 2u, 3u, 8u})
        for (uint32_t depth : {16u, 20u, 24u}) {
            size_t total[3] = {0, 0, 0}; uint64_t h[3] = {1469598103934665603ull, 1469598103934665603ull, 1469598103934665603ull};
            for (int sig = 0; sig < 6; ++sig)
                for (size_t li = 0; li < sizeof(lengths) / sizeof(lengths[0]); ++li)
                    for (int final = 0; final < 2; ++final) {
                        const size_t frames = lengths[li];
                        const uint32_t sb = depth == 16 ? 2 : 3;
                        // exact-size heap buffers: one byte read or written outside them is a sanitizer report
                        uint8_t* pcm = (uint8_t*)malloc(frames * ch * sb + (frames ? 0 : 1));
                        const uint64_t main_state = rng_state;                 // the added lengths draw from streams of their own
                        uint64_t* const own = (li >= n_effort1 || sig == 5) ? &lpc_state : li >= n_effort0 ? &extra_state : nullptr;
                        if (own) rng_state = *own;
                        memset(col_y, 0, sizeof col_y);
                        for (size_t i = 0; i < frames; ++i)
                            for (uint32_t c = 0; c < ch; ++c) {
                                int32_t v = sig == 5 ? coloured(c, depth) : sample(sig, i, c, frames, depth);
                                if (depth == 20) v = (int32_t)((uint32_t)v << 4) | (int32_t)(rng() & 15);
                                uint8_t* q = pcm + (i * ch + c) * sb;
                                q[0] = (uint8_t)v; q[1] = (uint8_t)(v >> 8); if (sb == 3) q[2] = (uint8_t)(v >> 16);
                            }
                        if (own) { *own = rng_state; rng_state = main_state; }
                        const size_t cap = d2d_flac_bound_bytes(ch, depth, frames, final);
                        uint8_t* out = (uint8_t*)malloc(cap ? cap : 1);
                        const uint32_t first = sig == 3 ? 0x7FFFFFFEu - (uint32_t)(frames / 4096) : (uint32_t)(0x7F * sig);
                        uint64_t bytes0 = 0, bytes1 = 0;
                        for (uint32_t ei = 0; ei < 3; ++ei) {
                            const uint32_t effort = efforts[ei];
                            d2d_flac_result r; size_t used = 0;
                            if (d2d_flac_encode_host_effort(ch, depth, effort, pcm, frames, first, final, out, cap, &r, &used) != D2D_OK) {
                                fprintf(stderr, "refused: %s\n", d2d_flac_error()); return 1;
                            }
                            if (r.bytes_out > cap || used > frames) { fprintf(stderr, "bound broken\n"); return 1; }
                            if (ei == 0) bytes0 = r.bytes_out;
                            else if (ei == 1) { bytes1 = r.bytes_out; if (bytes1 > bytes0) { fprintf(stderr, "effort 1 is longer than effort 0\n"); return 1; } }
                            else if (r.bytes_out > bytes1) { fprintf(stderr, "effort 12 is longer than effort 1\n"); return 1; }
                            // (the lines of efforts 0 and 1 cover what they always did: the five signals, their own lengths)
                            if (ei == 2 || (sig < 5 && (ei == 1 ? li < n_effort1 : li < n_effort0))) {
                                for (size_t i = 0; i < r.bytes_out; ++i) h[ei] = (h[ei] ^ out[i]) * 1099511628211ull;
                                total[ei] += r.bytes_out;
                            }
                            if (cap && d2d_flac_encode_host_effort(ch, depth, effort, pcm, frames, first, final, out, cap - 1, &r, &used) != D2D_ERR_CAPACITY) {
                                fprintf(stderr, "a capacity one byte short was accepted\n"); return 1;
                            }
                        }
                        free(pcm); free(out);
                    }
            printf("channels %u depth %u: %zu bytes, fnv %016llx\n", ch, depth, total[0], (unsigned long long)h[0]);
            printf("channels %u depth %u effort 1: %zu bytes, fnv %016llx\n", ch, depth, total[1], (unsigned long long)h[1]);
            printf("channels %u depth %u effort 12: %zu bytes, fnv %016llx\n", ch, depth, total[2], (unsigned long long)h[2]);
        }
    printf("ok\n");
    return 0;
}
