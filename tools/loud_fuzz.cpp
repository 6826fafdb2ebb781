// loud_fuzz.cpp -- the host twin of the loudness kernel and the integration behind it (dsd2dxd_amd/csrc/loud/d2d_loud_host.cpp on
// loud_meter.h: d2d_loud_measure_host, d2d_loud_create / _add / _finish) for a sanitizer build:
//   g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined -o loud_fuzz
//       tools/loud_fuzz.cpp dsd2dxd_amd/csrc/loud/d2d_loud_host.cpp dsd2dxd_amd/csrc/flac/d2d_flac_host.cpp && ./loud_fuzz SEED STREAMS
// CPU only (tests/test_loudness_cpu.py builds and runs it).  Every stream is seeded random PCM of a random depth, channel count, rate and
// length.  It is measured once in one final call, and once cut into calls at random frames: each call's PCM begins exactly at the
// minimum pre-roll, frame max(0, next_subblock - 2) * S, and lies in a heap block of exactly its size, as do its cells, so a read or
// write outside them is a sanitizer report.  CUT-INVARIANCE: the cells of the cut stream must be the other's bytes, the counts must add
// up, and the two meters must finish with the same bytes.  Prints "fuzz ok" at the end.
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

int main(int argc, char** argv) {
    rng_state = 0x9E3779B97F4A7C15ull ^ (argc > 1 ? strtoull(argv[1], 0, 10) : 1);
    const uint32_t streams = argc > 2 ? (uint32_t)strtoul(argv[2], 0, 10) : 100;
    static const uint32_t depths[4] = {16, 20, 24, 32}, chans[5] = {1, 2, 3, 6, 8}, rates[3] = {8000, 8010, 11020};
    uint64_t calls = 0, rows_seen = 0;
    for (uint32_t s = 0; s < streams; ++s) {
        const uint32_t depth = depths[rng() % 4], ch = chans[rng() % 5], rate = rates[rng() % 3];
        const size_t S = rate / 10, fb = (size_t)ch * (depth == 16 ? 2 : depth == 32 ? 4 : 3);
        const size_t frames = rng() % 6 == 0 ? rng() % 3 : rng() % (7 * S);
        std::vector<uint8_t> pcm(frames * fb);
        for (auto& b : pcm) b = (uint8_t)rng();
        if (depth == 32)                                             // finite floats of a sensible size: the top exponent bits cleared
            for (size_t i = 3; i < pcm.size(); i += 4) pcm[i] &= 0xBF;
        // the whole stream in one final call
        const size_t cap = (frames / S + 1) * ch;
        std::vector<d2d_loud_cell> whole(cap + 1);
        d2d_loud_io one{};
        one.pcm = pcm.data(); one.frames = frames; one.final = 1; one.cells = whole.data(); one.cells_capacity = cap;
        if (d2d_loud_measure_host(ch, depth, rate, &one) != D2D_OK) return fail(d2d_flac_error(), s, 0);
        if (frames && (one.subblocks != frames / S || one.cells_out != (frames / S + (frames % S ? 1 : 0)) * ch || one.next_subblock != frames / S))
            return fail("the counts of the single call", s, 0);
        d2d_loud *ma = nullptr, *mb = nullptr;
        if (d2d_loud_create(ch, rate, nullptr, &ma) != D2D_OK || d2d_loud_create(ch, rate, nullptr, &mb) != D2D_OK) return fail(d2d_flac_error(), s, 0);
        if (frames && d2d_loud_add(ma, whole.data(), one.subblocks, one.cells_out > one.subblocks * ch) != D2D_OK) return fail(d2d_flac_error(), s, 0);
        // ... and cut into calls
        uint64_t next = 0; size_t end = 0, rows = 0;
        for (bool last = frames == 0; !last;) {
            size_t take = rng() % 3 == 0 ? rng() % (2 * S) : rng() % (S / 2);
            if (rng() % 5 == 0) take = 0;
            if (end + take >= frames) { take = frames - end; last = true; }
            end += take;
            const uint64_t first = (next > 2 ? next - 2 : 0) * S;       // the minimum pre-roll and nothing more
            const size_t n = end - (size_t)first;
            uint8_t* piece = (uint8_t*)malloc(n ? n * fb : 1);
            memcpy(piece, pcm.data() + first * fb, n * fb);
            const size_t want_rows = end / S - (size_t)next + ((last && end % S) ? 1 : 0);
            d2d_loud_cell* cells = (d2d_loud_cell*)malloc(want_rows ? want_rows * ch * sizeof(d2d_loud_cell) : 1);
            d2d_loud_io io{};
            io.pcm = piece; io.frames = n; io.first_frame = first; io.first_subblock = next; io.final = last;
            io.cells = cells; io.cells_capacity = want_rows * ch; io.next_subblock = next;
            if (d2d_loud_measure_host(ch, depth, rate, &io) != D2D_OK) return fail(d2d_flac_error(), s, end);
            if (n && (io.cells_out != want_rows * ch || io.next_subblock != end / S)) return fail("the counts of a cut call", s, end);
            if (n) {
                if (memcmp(cells, whole.data() + rows * ch, io.cells_out * sizeof(d2d_loud_cell))) return fail("cells differ between the cuts", s, end);
                if (d2d_loud_add(mb, cells, io.subblocks, io.cells_out > io.subblocks * ch) != D2D_OK) return fail(d2d_flac_error(), s, end);
                rows += io.cells_out / ch; next = io.next_subblock;
            }
            free(piece); free(cells);
            ++calls;
        }
        if (rows * ch != (frames ? one.cells_out : 0)) return fail("the cut calls wrote another number of cells", s, frames);
        rows_seen += rows;
        d2d_loud_result ra, rb;
        memset(&ra, 0, sizeof(ra)); memset(&rb, 0, sizeof(rb));
        if (d2d_loud_finish(ma, &ra) != D2D_OK || d2d_loud_finish(mb, &rb) != D2D_OK) return fail(d2d_flac_error(), s, frames);
        if (memcmp(&ra, &rb, sizeof(ra))) return fail("the results differ between the cuts", s, frames);
        if (ra.blocks_total != (one.subblocks > 3 && frames ? one.subblocks - 3 : 0)) return fail("blocks_total", s, frames);
        d2d_loud_destroy(ma); d2d_loud_destroy(mb);
    }
    // refusals write nothing
    uint8_t some[64] = {0};
    d2d_loud_cell cells[8], same[8];
    memset(cells, 0xEE, sizeof(cells)); memcpy(same, cells, sizeof(cells));
    d2d_loud_io io{};
    io.pcm = some; io.frames = 4; io.cells = cells; io.cells_capacity = 8; io.final = 1;
    const d2d_loud_io before = io;
    if (d2d_loud_measure_host(2, 17, 8000, &io) != D2D_ERR_PARAM || d2d_loud_measure_host(0, 16, 8000, &io) != D2D_ERR_PARAM ||
        d2d_loud_measure_host(9, 16, 8000, &io) != D2D_ERR_PARAM || d2d_loud_measure_host(2, 16, 8005, &io) != D2D_ERR_PARAM ||
        d2d_loud_measure_host(2, 16, 7990, &io) != D2D_ERR_PARAM)
        return fail("a refusal's code", 0, 0);
    io.cells_capacity = 1;
    if (d2d_loud_measure_host(2, 16, 8000, &io) != D2D_ERR_CAPACITY) return fail("the capacity refusal's code", 0, 0);
    io = before; io.first_subblock = 3;                               // its pre-roll begins at frame 800, not at 0
    io.first_frame = 801;
    if (d2d_loud_measure_host(2, 16, 8000, &io) != D2D_ERR_PARAM) return fail("the pre-roll refusal's code", 0, 0);
    if (memcmp(cells, same, sizeof(cells))) return fail("a refusal wrote cells", 0, 0);
    printf("streams %u calls %llu rows %llu\nfuzz ok\n", streams, (unsigned long long)calls, (unsigned long long)rows_seen);
    return 0;
}
