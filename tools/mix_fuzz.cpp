// mix_fuzz.cpp -- the host half of the channel matrix under the host sanitizers: d2d_mix_frames_host (the CPU twin of the mix pass) and the
// "--mix" text parser, on random inputs.  Stand-alone: builds with g++ alone from this file and dsd2dxd_amd/csrc/mix/d2d_mix_host.cpp
// (tests/test_mix_cpu.py compiles it with -fsanitize=address,undefined and runs it).
//
//   mix_fuzz <seed> <rounds>
//
// Every round: a random mix inside the bounds (some at them, some outside, which must be refused), random sums up to the int32 range, a
// random epilogue.  The twin's frames are compared with a restatement in 128-bit integers of v and with the frames of the same call cut in
// two (the pass has no state but the index); exact-capacity buffers sit in heap blocks of exactly that size, so a byte too many is a
// sanitizer report.  The parser gets valid texts (whose coefficients must round-trip), random edits of them and random bytes.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <random>
#include <string>
#include <vector>

#include "../include/dsd2dxd_amd.h"
#include "../dsd2dxd_amd/csrc/mix/d2d_mix.h"
#include "../dsd2dxd_amd/csrc/mix/d2d_mix_text.h"

using namespace d2d;

static int die(const char* what, int round) { printf("FAIL round %d: %s\n", round, what); return 1; }

int main(int argc, char** argv) {
    const unsigned seed = argc > 1 ? (unsigned)atoi(argv[1]) : 1u;
    const int rounds = argc > 2 ? atoi(argv[2]) : 100;
    std::mt19937_64 rng(seed);
    auto uni = [&](int64_t lo, int64_t hi) { return (int64_t)(rng() % (uint64_t)(hi - lo + 1)) + lo; };
    const uint32_t depths[] = {16, 20, 24, 32};
    const char dithers[] = {'T', 'R', 'F', 'X'};
    for (int r = 0; r < rounds; ++r) {
        const uint32_t C = (uint32_t)uni(1, r % 7 == 0 ? 64 : 8), Co = (uint32_t)uni(1, C);
        const size_t frames = (size_t)uni(0, 300), stride = frames + (size_t)uni(0, 5);
        std::vector<int32_t> coef((size_t)Co * C);
        const int flavour = (int)uni(0, 5);
        for (uint32_t o = 0; o < Co; ++o) {
            int64_t left = MIX_ROW_MAX;
            for (uint32_t c = 0; c < C; ++c) {
                int64_t a = flavour == 0 ? (o == c ? MIX_UNITY : 0) : flavour == 1 ? MIX_COEF_MAX : uni(0, MIX_COEF_MAX);
                if (a > left) a = left;
                left -= a;
                coef[(size_t)o * C + c] = (int32_t)(uni(0, 1) ? a : -a);
            }
        }
        d2d_mix mix{(uint32_t)sizeof(d2d_mix), Co, coef.data()};
        if (mix_check(C, Co, coef.data())) return die("a mix inside the bounds was refused", r);
        std::vector<int32_t> sums(std::max<size_t>(stride * C, 1));
        for (auto& v : sums) v = flavour == 1 ? (uni(0, 1) ? INT32_MAX : INT32_MIN) : (int32_t)uni(INT32_MIN, INT32_MAX);
        const uint32_t bits = depths[uni(0, 3)], dither = (uint32_t)dithers[uni(0, 3)];
        const double level = (double)uni(-12, 6);
        const int S = (int)uni(20, 30);
        const uint64_t first = uni(0, 3) == 0 ? 0xFFFFFFFFull - (uint64_t)uni(0, 200) : (uint64_t)uni(0, 1 << 20), sd = rng();
        const size_t sb = bits == 16 ? 2 : bits == 32 ? 4 : 3, fb = sb * Co;
        // exact capacity, in a block of exactly that size
        uint8_t* whole = (uint8_t*)malloc(std::max<size_t>(frames * fb, 1));
        std::vector<double> pk(Co, 0.0);
        if (d2d_mix_frames_host(sums.data(), stride, frames, C, S, &mix, bits, dither, level, sd, first, whole, frames * fb, pk.data()) != D2D_OK)
            return die(d2d_mix_error(), r);
        if (frames && d2d_mix_frames_host(sums.data(), stride, frames, C, S, &mix, bits, dither, level, sd, first, whole, frames * fb - 1, nullptr) != D2D_ERR_CAPACITY)
            return die("a buffer one byte short was not refused", r);
        // the same frames in two calls
        const size_t cut = frames ? (size_t)uni(0, (int64_t)frames) : 0;
        uint8_t* a = (uint8_t*)malloc(std::max<size_t>(cut * fb, 1));
        uint8_t* b = (uint8_t*)malloc(std::max<size_t>((frames - cut) * fb, 1));
        std::vector<double> pk2(Co, 0.0);
        if (d2d_mix_frames_host(sums.data(), stride, cut, C, S, &mix, bits, dither, level, sd, first, a, cut * fb, pk2.data()) != D2D_OK ||
            d2d_mix_frames_host(sums.data() + cut, stride, frames - cut, C, S, &mix, bits, dither, level, sd, first + cut, b, (frames - cut) * fb, pk2.data()) != D2D_OK)
            return die(d2d_mix_error(), r);
        if (memcmp(whole, a, cut * fb) || memcmp(whole + cut * fb, b, (frames - cut) * fb)) return die("two calls differ from one", r);
        for (uint32_t o = 0; o < Co; ++o) if (pk[o] != pk2[o]) return die("peaks of two calls differ from one", r);
        // v in 128-bit integers, the peak from it
        const Epilogue epi = mix_epilogue(bits, dither, level, sd, Co);
        for (uint32_t o = 0; o < Co; ++o) {
            double want = 0.0;
            for (size_t n = 0; n < frames; ++n) {
                __int128 v = 0;
                for (uint32_t c = 0; c < C; ++c) v += (__int128)coef[(size_t)o * C + c] * (__int128)sums[(size_t)c * stride + n];
                if (v >= ((__int128)1 << 52) || v <= -((__int128)1 << 52)) return die("|v| reached 2^52 inside the bounds", r);
                const double y = ldexp((double)(int64_t)v, -(S + MIX_Q));
                want = fmax(want, fabs(y * epi.gain));
                uint32_t w = 0;
                memcpy(&w, whole + n * fb + o * sb, sb);
                if (w != (mix_sample_bits(epi, y, dither_word_at(dither_key64(sd, o), first + n)) & (sb == 4 ? 0xFFFFFFFFu : (1u << (8 * sb)) - 1u)))
                    return die("a sample differs from its restatement", r);
            }
            if (want != pk[o]) return die("a peak differs from its restatement", r);
        }
        free(whole); free(a); free(b);
        // outside the bounds: one coefficient too large, one row too heavy, too many rows
        {
            std::vector<int32_t> bad = coef;
            bad[(size_t)uni(0, (int64_t)bad.size() - 1)] = (int32_t)(MIX_COEF_MAX + 1 + uni(0, 1000)) * (uni(0, 1) ? 1 : -1);
            d2d_mix bm{(uint32_t)sizeof(d2d_mix), Co, bad.data()};
            uint8_t one[4];
            if (d2d_mix_frames_host(sums.data(), stride, 0, C, S, &bm, bits, dither, level, sd, first, one, 0, nullptr) != D2D_ERR_PARAM) return die("a coefficient above the bound passed", r);
            d2d_mix rows{(uint32_t)sizeof(d2d_mix), C + 1, coef.data()};
            if (d2d_mix_frames_host(sums.data(), stride, 0, C, S, &rows, bits, dither, level, sd, first, one, 0, nullptr) != D2D_ERR_PARAM) return die("more rows than channels passed", r);
            if (C >= 17) {
                std::vector<int32_t> heavy((size_t)C, 0);
                for (uint32_t c = 0; c < 16; ++c) heavy[c] = MIX_COEF_MAX;
                heavy[16] = 1;
                if (!mix_check(C, 1, heavy.data())) return die("a row above the bound passed", r);
            }
        }
        // the parser: a text of this mix's gains round-trips; edits and noise never crash and never pass the bounds
        {
            std::string text;
            for (uint32_t o = 0; o < Co; ++o) {
                for (uint32_t c = 0; c < C; ++c) {
                    char buf[64];
                    snprintf(buf, sizeof buf, "%s%.9f", c ? "," : "", (double)coef[(size_t)o * C + c] / 32768.0);
                    text += buf;
                }
                if (o + 1 < Co) text += ";";
            }
            std::vector<int32_t> back; uint32_t pr = 0, pc = 0; std::string err;
            if (!parse_mix_text(text.c_str(), back, pr, pc, err) || pr != Co || pc != C || back != coef) return die("a mix text did not round-trip", r);
            for (int k = 0; k < 20; ++k) {
                std::string t = text;
                const int edits = (int)uni(1, 4);
                for (int e = 0; e < edits && !t.empty(); ++e) {
                    const size_t at = (size_t)uni(0, (int64_t)t.size() - 1);
                    const char pool[] = "0123456789.,;-+e x\t";
                    if (uni(0, 2) == 0) t.erase(at, 1); else t[at] = uni(0, 9) == 0 ? (char)uni(1, 255) : pool[uni(0, (int64_t)sizeof(pool) - 2)];
                }
                if (parse_mix_text(t.c_str(), back, pr, pc, err)) {
                    if (back.size() != (size_t)pr * pc || mix_check(pc, pr, back.data())) return die("the parser passed a mix outside the bounds", r);
                } else if (err.empty()) return die("the parser refused without a reason", r);
            }
            if (parse_mix_text("", back, pr, pc, err) || parse_mix_text("1,2;3", back, pr, pc, err) || parse_mix_text("4.01", back, pr, pc, err) ||
                parse_mix_text("nan", back, pr, pc, err) || parse_mix_text("1,,2", back, pr, pc, err) || parse_mix_text(nullptr, back, pr, pc, err))
                return die("a malformed mix text passed", r);
            if (!parse_mix_text(" 0.5 , -0.5 ; 1,0", back, pr, pc, err) || back != std::vector<int32_t>{16384, -16384, 32768, 0}) return die("a plain mix text failed", r);
        }
    }
    printf("fuzz ok: %d rounds, seed %u\n", rounds, seed);
    return 0;
}
