// true_peak_fuzz.cpp -- the host twin of the true-peak kernel and the meter's true-peak side (dsd2dxd_amd/csrc/loud/d2d_loud_host.cpp on
// true_peak.h: d2d_true_peak_measure_host, d2d_loud_set_true_peak / _add_true_peaks / _true_peak) for a sanitizer build:
//   g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined -o true_peak_fuzz
//       tools/true_peak_fuzz.cpp dsd2dxd_amd/csrc/loud/d2d_loud_host.cpp dsd2dxd_amd/csrc/flac/d2d_flac_host.cpp && ./true_peak_fuzz SEED STREAMS
// CPU only (tests/test_true_peak_cpu.py builds and runs it).  Every stream is seeded random PCM of a random depth, channel count, rate
// and length.  It is measured once in one final call and held to a NAIVE LOOP written here from the definition (its own table, its own
// sample conversions); then it is cut into calls at random frames: each call's PCM begins exactly at the minimum history, frame
// max(0, next_subblock * S - 11), and lies in a heap block of exactly its size, as do its doubles, whose capacity is exactly what the
// call writes, so a read or write outside them is a sanitizer report; one frame of history less must be refused.  The doubles of the
// cut stream must be the other's bytes, the counts must add up, and both meters must report max(sample peak, largest double).  Prints
// "fuzz ok" at the end.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../include/dsd2dxd_amd.h"

static uint64_t rng_state;
static uint32_t rng() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return (uint32_t)(rng_state >> 16); }

static int fail(const char* what, uint32_t stream, uint64_t at) {
    printf("FAIL: %s (stream %u, frame %llu)\n", what, stream, (unsigned long long)at);
    return 1;
}

static const int P0[12] = {14, 90, -161, 272, -487, 1125, 7964, -838, 390, -218, 122, -68};
static const int P1[12] = {-239, 240, -424, 730, -1364, 3810, 6388, -1641, 832, -477, 271, -155};
static int coef(int p, int k) { return p == 0 ? P0[k] : p == 1 ? P1[k] : p == 2 ? P1[11 - k] : P0[11 - k]; }

static double value(const uint8_t* p, uint32_t depth) {
    if (depth == 16) return (double)(int16_t)(p[0] | (p[1] << 8)) / 32768.0;
    if (depth == 32) { float f; memcpy(&f, p, 4); return (double)f; }
    int32_t v = p[0] | (p[1] << 8) | (p[2] << 16);
    if (v & 0x800000) v -= 1 << 24;
    return (double)v / 8388608.0;
}

// the definition, frame by frame: rows of `ch` doubles, a partial last row
static std::vector<double> naive(const std::vector<uint8_t>& pcm, uint32_t ch, uint32_t depth, size_t S, size_t frames) {
    const size_t sb = depth == 16 ? 2 : depth == 32 ? 4 : 3, fb = ch * sb, rows = frames / S + (frames % S ? 1 : 0);
    std::vector<double> out(rows * ch, 0.0);
    for (size_t n = 0; n < frames; ++n)
        for (uint32_t c = 0; c < ch; ++c)
            for (int p = 0; p < 4; ++p) {
                double y = 0.0;
                for (int k = 0; k < 12; ++k)
                    if (n >= (size_t)k) y = y + (double)coef(p, k) * value(pcm.data() + (n - k) * fb + c * sb, depth);
                    else y = y + 0.0;
                const double v = fabs(y) / 8192.0;
                if (v > out[n / S * ch + c]) out[n / S * ch + c] = v;
            }
    return out;
}

int main(int argc, char** argv) {
    rng_state = 0x9E3779B97F4A7C15ull ^ (argc > 1 ? strtoull(argv[1], 0, 10) : 1);
    const uint32_t streams = argc > 2 ? (uint32_t)strtoul(argv[2], 0, 10) : 100;
    static const uint32_t depths[4] = {16, 20, 24, 32}, chans[5] = {1, 2, 3, 6, 8}, rates[3] = {8000, 8010, 11020};
    uint64_t calls = 0, rows_seen = 0;
    for (uint32_t s = 0; s < streams; ++s) {
        const uint32_t depth = depths[rng() % 4], ch = chans[rng() % 5], rate = rates[rng() % 3];
        const size_t S = rate / 10, fb = (size_t)ch * (depth == 16 ? 2 : depth == 32 ? 4 : 3);
        const size_t frames = rng() % 6 == 0 ? rng() % 14 : rng() % (5 * S);
        std::vector<uint8_t> pcm(frames * fb);
        for (auto& b : pcm) b = (uint8_t)rng();
        if (depth == 32)                                             // finite floats of a sensible size: the top exponent bits cleared
            for (size_t i = 3; i < pcm.size(); i += 4) pcm[i] &= 0xBF;
        // the whole stream in one final call, against the naive loop
        const size_t total = (frames / S + (frames % S ? 1 : 0)) * ch;
        double* whole = (double*)malloc(total ? total * sizeof(double) : 1);
        d2d_tpeak_io one{};
        one.pcm = pcm.data(); one.frames = frames; one.final = 1; one.peaks = whole; one.peaks_capacity = total;
        if (d2d_true_peak_measure_host(ch, depth, rate, &one) != D2D_OK) return fail(d2d_flac_error(), s, 0);
        if (frames && (one.subblocks != frames / S || one.peaks_out != total || one.next_subblock != frames / S)) return fail("the counts of the single call", s, 0);
        const std::vector<double> want = naive(pcm, ch, depth, S, frames);
        if (frames && memcmp(whole, want.data(), total * sizeof(double))) return fail("the twin differs from the naive loop", s, 0);
        // the cells of the same stream, for the meters
        std::vector<d2d_loud_cell> cells(total + 1);
        d2d_loud_io lone{};
        lone.pcm = pcm.data(); lone.frames = frames; lone.final = 1; lone.cells = cells.data(); lone.cells_capacity = total;
        if (d2d_loud_measure_host(ch, depth, rate, &lone) != D2D_OK) return fail(d2d_flac_error(), s, 0);
        d2d_loud *ma = nullptr, *mb = nullptr;
        if (d2d_loud_create(ch, rate, nullptr, &ma) != D2D_OK || d2d_loud_create(ch, rate, nullptr, &mb) != D2D_OK) return fail(d2d_flac_error(), s, 0);
        if (d2d_loud_set_true_peak(ma, 1) != D2D_OK || d2d_loud_set_true_peak(mb, 1) != D2D_OK) return fail(d2d_flac_error(), s, 0);
        const int partial = frames % S != 0;
        if (frames && d2d_loud_add(ma, cells.data(), lone.subblocks, partial) != D2D_OK) return fail(d2d_flac_error(), s, 0);
        if (frames && d2d_loud_add(mb, cells.data(), lone.subblocks, partial) != D2D_OK) return fail(d2d_flac_error(), s, 0);
        if (frames && d2d_loud_add_true_peaks(ma, whole, one.subblocks, partial) != D2D_OK) return fail(d2d_flac_error(), s, 0);
        if (frames && d2d_loud_set_true_peak(ma, 0) != D2D_ERR_PARAM) return fail("the switch moved after an add", s, 0);
        // ... and cut into calls
        uint64_t next = 0; size_t end = 0, rows = 0;
        for (bool last = frames == 0; !last;) {
            size_t take = rng() % 3 == 0 ? rng() % (2 * S) : rng() % (S / 2);
            if (rng() % 5 == 0) take = rng() % 13;
            if (end + take >= frames) { take = frames - end; last = true; }
            end += take;
            const uint64_t first = next * S > 11 ? next * S - 11 : 0;   // the minimum history and nothing more
            const size_t n = end - (size_t)first;
            uint8_t* piece = (uint8_t*)malloc(n ? n * fb : 1);
            memcpy(piece, pcm.data() + first * fb, n * fb);
            const size_t want_rows = end / S - (size_t)next + ((last && end % S) ? 1 : 0);
            double* peaks = (double*)malloc(want_rows ? want_rows * ch * sizeof(double) : 1);
            d2d_tpeak_io io{};
            io.pcm = piece; io.frames = n; io.first_frame = first; io.first_subblock = next; io.final = last;
            io.peaks = peaks; io.peaks_capacity = want_rows * ch; io.next_subblock = next;
            if (first && n > 1) {                                     // one frame of history less: refused, the record untouched
                d2d_tpeak_io less = io;
                less.pcm = piece + fb; less.frames = n - 1; less.first_frame = first + 1;
                const d2d_tpeak_io before = less;
                if (d2d_true_peak_measure_host(ch, depth, rate, &less) != D2D_ERR_PARAM || memcmp(&less, &before, sizeof(less))) return fail("a short history was not refused", s, end);
            }
            if (d2d_true_peak_measure_host(ch, depth, rate, &io) != D2D_OK) return fail(d2d_flac_error(), s, end);
            if (n && (io.peaks_out != want_rows * ch || io.next_subblock != end / S)) return fail("the counts of a cut call", s, end);
            if (n) {
                if (memcmp(peaks, whole + rows * ch, io.peaks_out * sizeof(double))) return fail("doubles differ between the cuts", s, end);
                if (d2d_loud_add_true_peaks(mb, peaks, io.subblocks, io.peaks_out > io.subblocks * ch) != D2D_OK) return fail(d2d_flac_error(), s, end);
                rows += io.peaks_out / ch; next = io.next_subblock;
            }
            free(piece); free(peaks);
            ++calls;
        }
        if (rows * ch != (frames ? one.peaks_out : 0)) return fail("the cut calls wrote another number of doubles", s, frames);
        rows_seen += rows;
        double ta = -1.0, tb = -1.0;
        if (!frames) {
            if (d2d_loud_true_peak(ma, &ta) != D2D_ERR_PARAM || ta != -1.0) return fail("a meter without rows gave a true peak", s, 0);
        } else {
            if (d2d_loud_true_peak(ma, &ta) != D2D_OK || d2d_loud_true_peak(mb, &tb) != D2D_OK) return fail(d2d_flac_error(), s, frames);
            d2d_loud_result r;
            if (d2d_loud_finish(ma, &r) != D2D_OK) return fail(d2d_flac_error(), s, frames);
            double top = r.peak;
            for (double v : want) if (v > top) top = v;
            if (ta != top || tb != top || ta < r.peak) return fail("the meter's true peak", s, frames);
        }
        d2d_loud_destroy(ma); d2d_loud_destroy(mb);
        free(whole);
    }
    // refusals write nothing
    uint8_t some[64] = {0};
    double peaks[8], same[8];
    memset(peaks, 0xEE, sizeof(peaks)); memcpy(same, peaks, sizeof(peaks));
    d2d_tpeak_io io{};
    io.pcm = some; io.frames = 4; io.peaks = peaks; io.peaks_capacity = 8; io.final = 1;
    const d2d_tpeak_io before = io;
    if (d2d_true_peak_measure_host(2, 17, 8000, &io) != D2D_ERR_PARAM || d2d_true_peak_measure_host(0, 16, 8000, &io) != D2D_ERR_PARAM ||
        d2d_true_peak_measure_host(9, 16, 8000, &io) != D2D_ERR_PARAM || d2d_true_peak_measure_host(2, 16, 8005, &io) != D2D_ERR_PARAM ||
        d2d_true_peak_measure_host(2, 16, 7990, &io) != D2D_ERR_PARAM)
        return fail("a refusal's code", 0, 0);
    io.peaks_capacity = 1;
    if (d2d_true_peak_measure_host(2, 16, 8000, &io) != D2D_ERR_CAPACITY) return fail("the capacity refusal's code", 0, 0);
    io = before; io.first_subblock = 1;                               // its history begins at frame 789
    io.first_frame = 790;
    if (d2d_true_peak_measure_host(2, 16, 8000, &io) != D2D_ERR_PARAM) return fail("the history refusal's code", 0, 0);
    if (memcmp(peaks, same, sizeof(peaks))) return fail("a refusal wrote doubles", 0, 0);
    printf("streams %u calls %llu rows %llu\nfuzz ok\n", streams, (unsigned long long)calls, (unsigned long long)rows_seen);
    return 0;
}
