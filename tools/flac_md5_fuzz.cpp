// flac_md5_fuzz.cpp -- the host twins of the GPU MD5 calls (d2d_flac_host.cpp on dsd2dxd_amd/csrc/flac/flac_md5.h: d2d_flac_md5_init_host,
// d2d_flac_md5_update_host, d2d_flac_md5_final_host) against the sink's own MD5 (dsd2dxd_amd/csrc/host/md5.h), for a sanitizer build:
//   g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined -o flac_md5_fuzz \
//       tools/flac_md5_fuzz.cpp dsd2dxd_amd/csrc/flac/d2d_flac_host.cpp && ./flac_md5_fuzz SEED MESSAGES
// CPU only (tests/test_flac_md5_cpu.py builds and runs it).  Every message is seeded random bytes of a random depth, channel count and
// length, fed in random splits of whole frames to both; each split's frames lie in a heap block of exactly their size, so a read outside
// them is a sanitizer report.  After every split the two must hold the same count and the same tail bytes, and the digest so far must be
// the sink's; the state record must be unchanged by the digest call.  Prints "fuzz ok" at the end.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../dsd2dxd_amd/csrc/host/md5.h"
#include "../include/dsd2dxd_amd.h"

static uint64_t rng_state;
static uint32_t rng() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return (uint32_t)(rng_state >> 16); }

static int fail(const char* what, uint32_t msg, size_t at) {
    printf("FAIL: %s (message %u, byte %zu)\n", what, msg, at);
    return 1;
}

int main(int argc, char** argv) {
    rng_state = 0x9E3779B97F4A7C15ull ^ (argc > 1 ? strtoull(argv[1], 0, 10) : 1);
    const uint32_t messages = argc > 2 ? (uint32_t)strtoul(argv[2], 0, 10) : 500;
    static const uint32_t depths[3] = {16, 20, 24}, chans[4] = {1, 2, 3, 8};
    uint64_t splits = 0, bytes = 0;
    for (uint32_t msg = 0; msg < messages; ++msg) {
        const uint32_t depth = depths[rng() % 3], ch = chans[rng() % 4], fb = ch * (depth == 16 ? 2 : 3);
        const size_t frames = rng() % 8 == 0 ? rng() % 3 : rng() % (1 + 20000 / fb);
        std::vector<uint8_t> pcm(frames * fb);
        for (auto& b : pcm) b = (uint8_t)rng();
        d2d_flac_md5_state st;
        memset(&st, 0xEE, sizeof(st));
        d2d_flac_md5_init_host(&st, 1);
        d2dhost::Md5 ref;
        for (size_t at = 0; at <= frames;) {
            // a split of 0 .. all remaining frames, short ones more often
            const size_t left = frames - at;
            size_t take = rng() % 4 == 0 ? left : rng() % 3 == 0 ? rng() % (left + 1) : rng() % (1 + (left < 40 ? left : 40));
            if (take > left) take = left;
            uint8_t* piece = (uint8_t*)malloc(take * fb ? take * fb : 1);             // exactly the split's bytes
            if (take) memcpy(piece, pcm.data() + at * fb, take * fb);
            if (d2d_flac_md5_update_host(ch, depth, take ? piece : nullptr, take, &st) != D2D_OK) return fail(d2d_flac_error(), msg, at * fb);
            if (depth == 20) {
                for (size_t i = 0; i < take * ch; ++i) {                                // the sink's own rule (FlacSink::write)
                    const int32_t v = (int32_t)((uint32_t)(piece[3 * i] | (piece[3 * i + 1] << 8) | (piece[3 * i + 2] << 16)) << 8) >> 12;
                    const uint8_t le[3] = {(uint8_t)v, (uint8_t)(v >> 8), (uint8_t)(v >> 16)};
                    ref.update(le, 3);
                }
            } else ref.update(piece, take * fb);
            free(piece);
            at += take; ++splits; bytes += take * fb;
            if (st.bytes != ref.len || st.tail_bytes != ref.fill || st.reserved != 0) return fail("count or tail length differ", msg, at * fb);
            if (memcmp(st.tail, ref.buf, ref.fill)) return fail("tail bytes differ", msg, at * fb);
            if (st.h[0] != ref.a || st.h[1] != ref.b || st.h[2] != ref.c || st.h[3] != ref.d) return fail("chaining values differ", msg, at * fb);
            const d2d_flac_md5_state before = st;
            uint8_t got[16], want[16];
            if (d2d_flac_md5_final_host(&st, got) != D2D_OK) return fail(d2d_flac_error(), msg, at * fb);
            if (memcmp(&before, &st, sizeof(st))) return fail("the digest call changed the state", msg, at * fb);
            d2dhost::Md5 copy = ref;
            copy.finish(want);
            if (memcmp(got, want, 16)) return fail("digests differ", msg, at * fb);
            if (at == frames && (take == 0 || rng() % 2)) break;
        }
    }
    // refusals write nothing
    d2d_flac_md5_state st, same;
    d2d_flac_md5_init_host(&st, 1);
    same = st;
    uint8_t some[48] = {0};
    if (d2d_flac_md5_update_host(2, 17, some, 4, &st) != D2D_ERR_PARAM || d2d_flac_md5_update_host(0, 16, some, 4, &st) != D2D_ERR_PARAM ||
        d2d_flac_md5_update_host(9, 16, some, 1, &st) != D2D_ERR_PARAM || d2d_flac_md5_update_host(2, 16, nullptr, 4, &st) != D2D_ERR_PARAM ||
        memcmp(&st, &same, sizeof(st)))
        return fail("a refusal", 0, 0);
    printf("messages %u splits %llu bytes %llu\nfuzz ok\n", messages, (unsigned long long)splits, (unsigned long long)bytes);
    return 0;
}
