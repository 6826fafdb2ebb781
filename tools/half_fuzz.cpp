// half_fuzz.cpp -- the host half of the 2:1 decimator under the host sanitizers: d2d_half_frames_host (the CPU twin of the half pass) and
// d2d_half_taps, on random inputs.  Stand-alone: builds with g++ alone from this file and dsd2dxd_amd/csrc/half/d2d_half_host.cpp
// (tests/test_half_cpu.py compiles it with -fsanitize=address,undefined and runs it).
//
//   half_fuzz <seed> <rounds>
//
// Every round: a batch of one to three files (some empty), random sums up to the int32 range (one round in four: +-INT32 extremes that follow
// the taps' signs), a random epilogue and first index of either parity.  The twin's frames are compared with a restatement of v in 128-bit
// integers and with the frames of the same stream cut in two calls, the history carried by hand; lines and exact-capacity buffers sit in
// heap blocks of exactly their size, so a sum read or a byte written too many is a sanitizer report.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <random>
#include <vector>

#include "../include/dsd2dxd_amd.h"
#include "../dsd2dxd_amd/csrc/half/d2d_half.h"

using namespace d2d;

static int die(const char* what, int round) { printf("FAIL round %d: %s\n", round, what); return 1; }

// a heap block of exactly n int32 / bytes (at least one, so that malloc(0) never decides)
template <class T> static T* block(size_t n) { return (T*)malloc(std::max<size_t>(n, 1) * sizeof(T)); }

int main(int argc, char** argv) {
    const unsigned seed = argc > 1 ? (unsigned)atoi(argv[1]) : 1u;
    const int rounds = argc > 2 ? atoi(argv[2]) : 100;
    std::mt19937_64 rng(seed);
    auto uni = [&](int64_t lo, int64_t hi) { return (int64_t)(rng() % (uint64_t)(hi - lo + 1)) + lo; };
    const uint32_t depths[] = {16, 20, 24, 32};
    const char dithers[] = {'T', 'R', 'F', 'X'};
    uint32_t nt = 0, tt = 0;
    int32_t taps[HALF_NT];
    if (d2d_half_taps(&nt, &tt, nullptr, 0) != D2D_OK || nt != (uint32_t)HALF_NT || tt != (uint32_t)HALF_T) return die("d2d_half_taps: sizes", -1);
    if (d2d_half_taps(&nt, &tt, taps, HALF_NT - 1) != D2D_ERR_CAPACITY || d2d_half_taps(&nt, &tt, taps, HALF_NT) != D2D_OK) return die("d2d_half_taps: capacity", -1);
    if (memcmp(taps, D2D_HALF_TAPS, sizeof taps)) return die("d2d_half_taps: the table", -1);
    for (int r = 0; r < rounds; ++r) {
        const uint32_t C = (uint32_t)uni(1, r % 9 == 0 ? 64 : 4), nfiles = (uint32_t)uni(1, 3);
        const uint32_t bits = depths[uni(0, 3)], dither = (uint32_t)dithers[uni(0, 3)];
        const double level = (double)uni(-12, 6);
        const int S = (int)uni(24, 30);
        const uint64_t sd = rng();
        const size_t sb = bits == 16 ? 2 : bits == 32 ? 4 : 3, fb = sb * C;
        const Epilogue epi = mix_epilogue(bits, dither, level, sd, C);
        const int flavour = (int)uni(0, 3);
        std::vector<d2d_half_job> jobs(nfiles);
        std::vector<int32_t*> lines(nfiles);
        std::vector<uint8_t*> pcm(nfiles);
        std::vector<std::vector<double>> pk(nfiles, std::vector<double>(C, 0.0));
        for (uint32_t f = 0; f < nfiles; ++f) {
            const size_t n = uni(0, 3) == 0 ? 0 : (size_t)uni(0, 900), stride = HALF_HIST + n;
            const uint64_t first = uni(0, 3) == 0 ? 2 * (0xFFFFFFFFull - (uint64_t)uni(0, 300)) + (uint64_t)uni(0, 1) : (uint64_t)uni(0, 1 << 20);
            lines[f] = block<int32_t>(stride * C);
            for (size_t i = 0; i < stride * C; ++i) lines[f][i] = (int32_t)uni(INT32_MIN, INT32_MAX);
            if (flavour == 0 && n) {           // one frame's window at the extremes, following the taps' signs (either sign of v)
                const uint64_t k = half_frames_after(first) + (uint64_t)uni(0, (int64_t)((n + 1) / 2));
                const int64_t centre = (int64_t)(2 * k - first) + (int64_t)HALF_HIST, sgn = uni(0, 1) ? 1 : -1;
                for (uint32_t c = 0; c < C; ++c)
                    for (int j = 0; j < HALF_NT; ++j) {
                        const int64_t at = centre - j;
                        if (at >= 0 && at < (int64_t)stride) lines[f][c * stride + (size_t)at] = (int32_t)(((D2D_HALF_TAPS[j] < 0) ? -sgn : sgn) * (int64_t)INT32_MAX);
                    }
            }
            const uint64_t frames = half_frames_after(first + n) - half_frames_after(first);
            pcm[f] = block<uint8_t>(frames * fb);
            jobs[f] = d2d_half_job{lines[f], stride, n, first, pcm[f], (size_t)frames * fb, pk[f].data(), 0};
        }
        if (d2d_half_frames_host(jobs.data(), nfiles, C, S, bits, dither, level, sd) != D2D_OK) return die(d2d_half_error(), r);
        for (uint32_t f = 0; f < nfiles; ++f) {
            const d2d_half_job& j = jobs[f];
            const uint64_t k0 = half_frames_after(j.first_index);
            if (j.frames_out != half_frames_after(j.first_index + j.n) - k0) return die("frames_out", r);
            // a buffer one byte short is refused, and nothing is written
            if (j.frames_out) {
                d2d_half_job s = j;
                s.pcm_capacity_bytes -= 1; s.peaks = nullptr;
                if (d2d_half_frames_host(&s, 1, C, S, bits, dither, level, sd) != D2D_ERR_CAPACITY) return die("a buffer one byte short was not refused", r);
            }
            // v in 128-bit integers, the sample and the peak from it
            for (uint32_t c = 0; c < C; ++c) {
                double want = 0.0;
                const int32_t* x = j.sums + (size_t)c * j.stride + HALF_HIST;
                for (size_t t = 0; t < j.frames_out; ++t) {
                    const uint64_t k = k0 + t;
                    const ptrdiff_t at = (ptrdiff_t)(2 * k - j.first_index);
                    __int128 v = 0;
                    for (int q = 0; q < HALF_NT; ++q) v += (__int128)D2D_HALF_TAPS[q] * (__int128)x[at - q];
                    if (v >= ((__int128)1 << 59) || v <= -((__int128)1 << 59)) return die("|v| reached 2^59", r);
                    __int128 w = v + ((__int128)1 << (HALF_T - 1));
                    w = w >= 0 ? w >> HALF_T : -((-w + (((__int128)1 << HALF_T) - 1)) >> HALF_T);       // floor, without shifting a negative value
                    const double y = ldexp((double)(int64_t)w, -S);
                    want = fmax(want, fabs(y * epi.gain));
                    uint32_t got = 0;
                    memcpy(&got, (const uint8_t*)j.pcm + t * fb + c * sb, sb);
                    if (got != (mix_sample_bits(epi, y, dither_word_at(dither_key64(sd, c), k)) & (sb == 4 ? 0xFFFFFFFFu : (1u << (8 * sb)) - 1u)))
                        return die("a sample differs from its restatement", r);
                }
                if (want != pk[f][c]) return die("a peak differs from its restatement", r);
            }
            // the same stream in two calls, each line in a block of its own size, the history carried by hand
            const size_t cut = j.n ? (size_t)uni(0, (int64_t)j.n) : 0;
            const size_t sa = HALF_HIST + cut, sbk = HALF_HIST + (j.n - cut);
            int32_t* la = block<int32_t>(sa * C);
            int32_t* lb = block<int32_t>(sbk * C);
            for (uint32_t c = 0; c < C; ++c) {
                memcpy(la + c * sa, j.sums + c * j.stride, sa * sizeof(int32_t));
                memcpy(lb + c * sbk, j.sums + c * j.stride + cut, sbk * sizeof(int32_t));
            }
            const uint64_t fa = half_frames_after(j.first_index + cut) - k0, fbk = j.frames_out - fa;
            uint8_t* pa = block<uint8_t>(fa * fb);
            uint8_t* pb = block<uint8_t>(fbk * fb);
            std::vector<double> pk2(C, 0.0);
            d2d_half_job two[2] = {{la, sa, cut, j.first_index, pa, (size_t)fa * fb, pk2.data(), 0},
                                   {lb, sbk, j.n - cut, j.first_index + cut, pb, (size_t)fbk * fb, pk2.data(), 0}};
            if (d2d_half_frames_host(&two[0], 1, C, S, bits, dither, level, sd) != D2D_OK || d2d_half_frames_host(&two[1], 1, C, S, bits, dither, level, sd) != D2D_OK)
                return die(d2d_half_error(), r);
            if (two[0].frames_out != fa || two[1].frames_out != fbk) return die("frames of two calls", r);
            if (memcmp(j.pcm, pa, fa * fb) || memcmp((const uint8_t*)j.pcm + fa * fb, pb, fbk * fb)) return die("two calls differ from one", r);
            for (uint32_t c = 0; c < C; ++c) if (pk[f][c] != pk2[c]) return die("peaks of two calls differ from one", r);
            free(la); free(lb); free(pa); free(pb);
        }
        // what the checks refuse
        {
            d2d_half_job bad = jobs[0];
            if (d2d_half_frames_host(&bad, 1, 0, S, bits, dither, level, sd) != D2D_ERR_PARAM || d2d_half_frames_host(&bad, 1, 65, S, bits, dither, level, sd) != D2D_ERR_PARAM)
                return die("a bad channel count passed", r);
            if (d2d_half_frames_host(&bad, 1, C, S, 12, dither, level, sd) != D2D_ERR_PARAM || d2d_half_frames_host(&bad, 1, C, S, bits, 'N', level, sd) != D2D_ERR_PARAM)
                return die("a bad depth or dither passed", r);
            if (bad.n) { bad.stride = HALF_HIST + bad.n - 1; if (d2d_half_frames_host(&bad, 1, C, S, bits, dither, level, sd) != D2D_ERR_PARAM) return die("a short line passed", r); }
        }
        for (uint32_t f = 0; f < nfiles; ++f) { free(lines[f]); free(pcm[f]); }
    }
    printf("fuzz ok: %d rounds, seed %u\n", rounds, seed);
    return 0;
}
