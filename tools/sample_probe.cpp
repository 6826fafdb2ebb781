// sample_probe.cpp -- the per-sample arithmetic of dsd2dxd_amd/csrc/d2d_sample.h on the host (tests/test_sample_arithmetic.py).
//   g++ -O2 -std=c++17 -ffp-contract=off -o sample_probe sample_probe.cpp
//   sample_probe rng KEY KSTEP LO0 LO COUNT     dither_word(lo, ...) for lo = LO, LO + 1, ... (mod 2^32), one per line
//   sample_probe requant KIND F BITS SEED N     requant_int<KIND> against the f64 definition of the same header
//   sample_probe quant SEED N                   round_clip / dither_float against the epilogue as it was first written down
// The last two print "cases <n> mismatches <m>" and the first few mismatches.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../dsd2dxd_amd/csrc/d2d_sample.h"

using namespace d2d;

static uint64_t rng_state;
static uint64_t next64() {      // splitmix64
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// the definition: x = v * 2^-F exactly, one f64 addition of the dither, round half away from zero, clip
template <int KIND>
static int32_t requant_f64(int32_t v, int F, uint32_t z, int bits) {
    const double x = ldexp((double)v, -F);
    return round_clip(x + dither_f64<KIND>(dither_term<KIND>(z)), ldexp(1.0, bits - 1));
}

template <int KIND>
static int run_requant(int F, int bits, uint64_t nrandom) {
    const int64_t rail = (int64_t)1 << (bits - 1 + F);          // v at x = 2^(bits-1); past int32 where bits - 1 + F > 31
    const int64_t lsb = (int64_t)1 << F, half = (int64_t)1 << (F - 1);
    std::vector<int64_t> vs = {0, 1, -1, INT32_MAX, INT32_MAX - 1, INT32_MIN, INT32_MIN + 1};
    // within 3 LSB of both rails (of the ends of int32 where a rail lies outside it), every v
    for (int64_t c : {rail, -rail, rail - lsb, -rail - lsb, (int64_t)INT32_MAX - 3 * lsb, (int64_t)INT32_MIN + 3 * lsb})
        for (int64_t d = -3 * lsb - 2; d <= 3 * lsb + 2; ++d) vs.push_back(c + d);
    // exact ties: multiples of 2^(F-1), around zero, around the rails and anywhere
    for (int64_t k = -3000; k <= 3000; ++k) { vs.push_back(k * half); vs.push_back(rail + k * half); vs.push_back(-rail + k * half); }
    for (int i = 0; i < 20000; ++i) vs.push_back((int64_t)(int32_t)next64() / half * half);
    const int64_t span = std::min<int64_t>(rail + rail / 4, INT32_MAX);
    for (uint64_t i = 0; i < nrandom; ++i) {
        const uint64_t r = next64();
        // half of them anywhere in int32, half inside 1.25 times the range of the depth (where int32 reaches that far)
        vs.push_back((i & 1) ? (int64_t)(int32_t)r : (int64_t)(r % (uint64_t)(2 * span + 1)) - span);
    }
    const int32_t qmax = (int32_t)((1u << (bits - 1)) - 1u), qmin = -qmax - 1;
    uint64_t cases = 0, bad = 0;
    for (int64_t v64 : vs) {
        if (v64 < INT32_MIN || v64 > INT32_MAX) continue;
        const int32_t v = (int32_t)v64;
        const uint32_t zs[3] = {(uint32_t)next64(), 0u, 0xFFFFFFFFu};
        for (int zi = 0; zi < (KIND == DITHER_NONE ? 1 : 3); ++zi) {
            const int32_t a = requant_int<KIND>(v, F, zs[zi], qmin, qmax), b = requant_f64<KIND>(v, F, zs[zi], bits);
            ++cases;
            if (a != b && bad++ < 8) printf("mismatch v %d z %u: integer %d, f64 %d\n", v, zs[zi], a, b);
        }
    }
    printf("cases %llu mismatches %llu\n", (unsigned long long)cases, (unsigned long long)bad);
    return 0;
}

// ---- the epilogue as d2d_device.h first stated it, kept here word for word as the yardstick of the shared pieces ----
static int32_t first_quantise_int(double scale, int dither, int bits, double y, uint32_t rnd) {
    const double x = y * scale;
    double d = 0.0;
    if (dither == 'T') d = (double)((rnd & 0xFFFFu) + (rnd >> 16) + 1u) * 0x1p-16 - 1.0;
    else if (dither == 'R') d = (double)(2u * (rnd >> 16) + 1u) * 0x1p-17 - 0.5;
    const double q = x + d;
    const double r = trunc(q + copysign(0.5, q));
    const int32_t lim = 1 << (bits - 1);
    int32_t iv = (int32_t)fmax(fmin(r, 2147483520.0), -2147483648.0);
    iv = std::min(std::max(iv, -lim), lim - 1);
    return iv;
}
static float first_quantise_f32(double gain, int dither, double y, uint32_t rnd) {
    double x = y * gain;
    if (dither == 'F') {
        const float f = (float)x;
        uint32_t fb;
        memcpy(&fb, &f, 4);
        const int e = (int)((fb >> 23) & 0xFF);
        const int expon = e ? e - 126 : 0;
        const double t = ((double)rnd - 2147483647.0) * 5.5e-36;
        x = x + ldexp(t, expon + 62);
    }
    return (float)x;
}

static int run_quant(uint64_t n) {
    std::vector<double> ys = {0.0, -0.0, 1.0, -1.0, 0.5, -0.5, 1.0 - 0x1p-53, -1.0 - 0x1p-52, 1e-300, -1e-300, 4.0, -4.0,
                              0x1p-126, -0x1p-126, 0x1p-127, -0x1p-149, 0x1p-150, 1.5 * 0x1p-140, -1.25 * 0x1p-130, 0x1p-126 - 0x1p-160};
    for (int bits : {16, 20, 24})        // at the clip and at the ties next to it
        for (int k = -6; k <= 6; ++k)
            for (double s : {1.0, -1.0}) ys.push_back(s * (1.0 + k * ldexp(0.25, -(bits - 1))));
    while (ys.size() < n) {
        const uint64_t r = next64();
        const double u = (double)(int64_t)next64() * 0x1p-63;                   // [-1, 1)
        ys.push_back((r & 3) == 0 ? u * 1.5 : (r & 3) == 1 ? ldexp(u, -(int)((r >> 8) % 160)) : u);
    }
    uint64_t cases = 0, bad = 0;
    for (double y : ys) {
        const uint32_t rnd = (uint32_t)next64();
        for (double gain : {1.0, 0.5011872336272722, 1.9952623149688795}) {
            for (int bits : {16, 20, 24}) {
                const double scale = gain * (double)(1u << (bits - 1)), lim = (double)(1u << (bits - 1));
                const double x = y * scale;
                const int32_t want[3] = {first_quantise_int(scale, 'X', bits, y, rnd), first_quantise_int(scale, 'T', bits, y, rnd),
                                         first_quantise_int(scale, 'R', bits, y, rnd)};
                const int32_t got[3] = {round_clip(x + dither_f64<DITHER_NONE>(dither_term<DITHER_NONE>(rnd)), lim),
                                        round_clip(x + dither_f64<DITHER_TRI>(dither_term<DITHER_TRI>(rnd)), lim),
                                        round_clip(x + dither_f64<DITHER_RECT>(dither_term<DITHER_RECT>(rnd)), lim)};
                for (int i = 0; i < 3; ++i) {
                    ++cases;
                    if (want[i] != got[i] && bad++ < 8) printf("mismatch int y %a bits %d kind %d: %d, first form %d\n", y, bits, i, got[i], want[i]);
                }
            }
            const float wf = first_quantise_f32(gain, 'F', y, rnd), gf = (float)dither_float(y * gain, rnd);
            ++cases;
            if (f32_bits(wf) != f32_bits(gf) && bad++ < 8) printf("mismatch float y %a: %a, first form %a\n", y, gf, wf);
        }
    }
    printf("cases %llu mismatches %llu\n", (unsigned long long)cases, (unsigned long long)bad);
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 7 && !strcmp(argv[1], "rng")) {
        const uint32_t key = (uint32_t)strtoull(argv[2], 0, 0), kstep = (uint32_t)strtoull(argv[3], 0, 0), lo0 = (uint32_t)strtoull(argv[4], 0, 0);
        uint32_t lo = (uint32_t)strtoull(argv[5], 0, 0);
        for (uint64_t i = 0, n = strtoull(argv[6], 0, 0); i < n; ++i, ++lo) printf("%u\n", dither_word(lo, key, kstep, lo0));
        return 0;
    }
    if (argc == 7 && !strcmp(argv[1], "requant")) {
        const int kind = atoi(argv[2]), F = atoi(argv[3]), bits = atoi(argv[4]);
        rng_state = strtoull(argv[5], 0, 0);
        const uint64_t n = strtoull(argv[6], 0, 0);
        if (F < 1 || F > 16 || bits < 2 || bits > 32) return 2;
        return kind == DITHER_TRI ? run_requant<DITHER_TRI>(F, bits, n) : kind == DITHER_RECT ? run_requant<DITHER_RECT>(F, bits, n)
                                                                                              : run_requant<DITHER_NONE>(F, bits, n);
    }
    if (argc == 4 && !strcmp(argv[1], "quant")) {
        rng_state = strtoull(argv[2], 0, 0);
        return run_quant(strtoull(argv[3], 0, 0));
    }
    fprintf(stderr, "usage: sample_probe rng KEY KSTEP LO0 LO COUNT | requant KIND F BITS SEED N | quant SEED N\n");
    return 2;
}
