// segments_fuzz.cpp -- the host twins of the segment calls (include/dsd2dxd_amd.h, "A chunk's bookkeeping in one launch") under the
// sanitisers: random segment lists against a bytewise model, the overlap check against its quadratic definition, the offsets
// arithmetic of the pack.  Stand-alone, no HIP:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -o segments_fuzz tools/segments_fuzz.cpp \
//       dsd2dxd_amd/csrc/batch/d2d_segments_host.cpp dsd2dxd_amd/csrc/flac/d2d_flac_host.cpp && ./segments_fuzz 400
// Every buffer is a heap block of its exact size, so a byte read or written outside a declared range is the address sanitiser's.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../include/dsd2dxd_amd.h"

static uint64_t state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() { state ^= state << 13; state ^= state >> 7; state ^= state << 17; return state; }
static size_t below(size_t n) { return n ? (size_t)(rnd() % n) : 0; }

#define REQUIRE(cond) do { if (!(cond)) { printf("FAILED %s, line %d (round %d)\n", #cond, __LINE__, round_no); return 1; } } while (0)
static int round_no = 0;

// the definition: a dst range of non-zero length shares a byte with a src range or another dst range
static bool overlaps(const std::vector<d2d_segment>& s) {
    auto meet = [](const void* a, size_t na, const void* b, size_t nb) {
        const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
        return na && nb && x < y + nb && y < x + na;
    };
    for (size_t i = 0; i < s.size(); ++i)
        for (size_t j = 0; j < s.size(); ++j) {
            if (meet(s[i].dst, s[i].bytes, s[j].src, s[j].bytes)) return true;
            if (i != j && meet(s[i].dst, s[i].bytes, s[j].dst, s[j].bytes)) return true;
        }
    return false;
}

static int move_round() {
    // one arena; segments thrown at it: some lists overlap, some do not
    const size_t arena = 64 + below(4000);
    std::vector<uint8_t> mem(arena), before, model;
    for (auto& b : mem) b = (uint8_t)rnd();
    std::vector<d2d_segment> s(below(12));
    const bool disjoint = rnd() & 1;                             // disjoint: slots of the arena dealt out in order, so most lists pass
    size_t at = 0;
    for (auto& g : s) {
        if (disjoint) {
            const size_t room = (arena - at) / 2, n = below(room / 2 + 1), gap = below(4);
            g.src = mem.data() + at; g.dst = mem.data() + at + n + gap; g.bytes = n + gap + n <= arena - at ? n : 0;
            at += g.bytes ? 2 * n + gap : 0;
        } else {
            g.bytes = below(arena / 4);
            g.src = mem.data() + below(arena - g.bytes + 1); g.dst = mem.data() + below(arena - g.bytes + 1);
        }
    }
    before = mem; model = mem;
    const bool bad = overlaps(s);
    for (const auto& g : s)
        for (size_t i = 0; i < g.bytes; ++i) model[(uint8_t*)g.dst - mem.data() + i] = before[(const uint8_t*)g.src - mem.data() + i];
    const int rc = d2d_segments_move_host(s.data(), (uint32_t)s.size());
    REQUIRE(rc == (bad ? D2D_ERR_PARAM : D2D_OK));
    REQUIRE(mem == (bad ? before : model));
    return 0;
}

static int pack_round() {
    const uint32_t n = (uint32_t)below(20);
    std::vector<std::vector<uint8_t>> data(n);
    std::vector<uint64_t> len(n);
    std::vector<d2d_pack_src> src(n);
    size_t cap = 0, total = 0;
    const uint32_t too_long = (rnd() % 4 == 0 && n) ? (uint32_t)below(n) : n;      // n: none
    for (uint32_t k = 0; k < n; ++k) {
        const size_t bytes = rnd() % 3 ? below(300) : 0, slack = below(3);
        data[k].reserve(1);                                        // (a base is non-null where max_bytes > 0, whatever the length turns out to be)
        data[k].resize(bytes);
        for (auto& b : data[k]) b = (uint8_t)rnd();
        len[k] = bytes; src[k].base = data[k].data(); src[k].bytes = &len[k]; src[k].max_bytes = bytes + slack;
        if (k == too_long) len[k] = src[k].max_bytes + 1 + below(5);
        cap += src[k].max_bytes; total += bytes;
    }
    std::vector<uint8_t> dst(cap, 0xEE), dst0 = dst;
    // the table at any alignment: the twin reads and writes it bytewise
    std::vector<uint8_t> raw(8 * ((size_t)n + 1) + 8);
    uint64_t* offsets = (uint64_t*)(raw.data() + below(8));
    if (cap) REQUIRE(d2d_segments_pack_host(src.data(), n, dst.data(), cap - 1, offsets) == D2D_ERR_CAPACITY);
    REQUIRE(dst == dst0);
    REQUIRE(d2d_segments_pack_host(src.data(), n, cap ? dst.data() : nullptr, cap, offsets) == D2D_OK);
    uint64_t off = 0;
    for (uint32_t k = 0; k <= n; ++k) {
        uint64_t got;
        memcpy(&got, (const uint8_t*)offsets + 8 * (size_t)k, 8);
        if (too_long < n) { REQUIRE(got == UINT64_MAX); continue; }
        REQUIRE(got == off);
        if (k < n) {
            REQUIRE(len[k] == 0 || memcmp(dst.data() + off, data[k].data(), (size_t)len[k]) == 0);
            off += len[k];
        }
    }
    if (too_long < n) REQUIRE(dst == dst0);
    else {
        REQUIRE(off == total);
        for (size_t i = total; i < cap; ++i) REQUIRE(dst[i] == 0xEE);
    }
    return 0;
}

int main(int argc, char** argv) {
    const int rounds = argc > 1 ? atoi(argv[1]) : 200;
    // the refusals that need no memory
    d2d_segment wrap{(void*)(uintptr_t)-8, (const void*)(uintptr_t)64, 16};
    if (d2d_segments_move_host(&wrap, 1) != D2D_ERR_PARAM || d2d_segments_move_host(nullptr, 1) != D2D_ERR_PARAM ||
        d2d_segments_move_host(nullptr, 0) != D2D_OK || d2d_segments_pack_host(nullptr, 0, nullptr, 0, nullptr) != D2D_ERR_PARAM) {
        printf("FAILED the refusals\n");
        return 1;
    }
    for (round_no = 0; round_no < rounds; ++round_no)
        if (move_round() || pack_round()) return 1;
    printf("segments fuzz ok: %d rounds\n", rounds);
    return 0;
}
