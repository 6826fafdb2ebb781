// d2d_flac_host.cpp -- the host half of the FLAC entry points: sizes, the error slot, d2d_flac_encode_host, which is the sink's
// own frame encoder (flac_frame_enc.h) behind the C ABI, and the readers on flac_parse.h: d2d_flac_decode_host and d2d_flac_verify_host,
// the CPU twin of the GPU verify call; and the CPU twins of the GPU MD5 calls on flac_md5.h.  No HIP: tools and tests build this file
// with g++ alone.
#include <string.h>

#include <algorithm>
#include <vector>

#include "d2d_flac_internal.h"
#include "flac_expect.h"
#include "flac_frame_enc.h"
#include "flac_md5.h"

namespace d2dflac {

static thread_local std::string g_flac_error;
int fail(int code, const std::string& message) { g_flac_error = message; return code; }

const char* reason_name(uint32_t reason) {
    static const char* const names[] = {"none", "SIZE", "HEADER", "CRC8", "CRC16", "UNSUPPORTED", "SYNTAX", "LENGTH", "SAMPLES"};
    return reason < sizeof(names) / sizeof(names[0]) ? names[reason] : "?";
}

}  // namespace d2dflac

using namespace d2dflac;

namespace {

// the decoder's side of flac_parse.h: keeps the coded signals of one frame, then undoes the stereo assignment
struct DecodeSig {
    std::vector<int32_t> x[8];
    int32_t store[2 * d2dparse::MAX_LPC_ORDER];
    uint32_t s = 0;
    void begin(uint32_t subframe, uint32_t) { s = subframe; x[s].clear(); }
    bool put(uint32_t, int32_t v) { x[s].push_back(v); return true; }
    int32_t& hist(uint32_t k) { return store[k]; }
    int32_t& coef(uint32_t k) { return store[d2dparse::MAX_LPC_ORDER + k]; }
    // rule 8: left and right from the assignment; false where one does not fit the depth
    bool undo_stereo(uint32_t assignment, uint32_t n, uint32_t depth) {
        if (assignment < 8) return true;
        const int64_t lo = -((int64_t)1 << (depth - 1)), hi = ((int64_t)1 << (depth - 1)) - 1;
        for (uint32_t i = 0; i < n; ++i) {
            int64_t l, r;
            if (assignment == 8) { l = x[0][i]; r = l - x[1][i]; }
            else if (assignment == 9) { r = x[1][i]; l = r + x[0][i]; }
            else { const int64_t side = x[1][i], mid = (int64_t)x[0][i] * 2 + (side & 1); l = (mid + side) >> 1; r = (mid - side) >> 1; }
            if (l < lo || l > hi || r < lo || r > hi) return false;
            x[0][i] = (int32_t)l; x[1][i] = (int32_t)r;
        }
        return true;
    }
};

void clean_record(d2d_flac_check& c) { c = d2d_flac_check{0, 0, 0, 0xFFFFFFFFu, D2D_FLAC_BAD_NONE}; }
void count_block(d2d_flac_check& c, uint32_t b, uint32_t reason, uint32_t n) {
    ++c.blocks_checked;
    if (!reason) { c.samples_checked += n; return; }
    if (c.bad_blocks++ == 0) { c.first_bad_block = b; c.first_bad_reason = reason; }
}

}  // namespace

extern "C" {

const char* d2d_flac_error(void) { return g_flac_error.c_str(); }

size_t d2d_flac_bound_bytes(uint32_t channels, uint32_t bit_depth, size_t frames, int final) {
    if (!depth_ok(bit_depth) || channels == 0 || channels > 8) return 0;
    const uint32_t rem = (uint32_t)(frames % BS);
    return (frames / BS) * frame_bound(channels, bit_depth, BS) + ((final && rem) ? frame_bound(channels, bit_depth, rem) : 0);
}

size_t d2d_flac_workspace_bytes(uint32_t channels, uint32_t bit_depth, size_t frames, int final) {
    if (!depth_ok(bit_depth) || channels == 0 || channels > 8) return 0;
    const size_t blocks = block_count(frames, final);
    return align16(4 * blocks) + blocks * slot_bytes(channels, bit_depth);
}

int d2d_flac_encode_host(uint32_t channels, uint32_t bit_depth, const void* pcm, size_t frames, uint32_t first_block, int final,
                         void* out, size_t out_capacity_bytes, d2d_flac_result* result, size_t* frames_consumed) {
    return d2d_flac_encode_host_effort(channels, bit_depth, D2D_FLAC_EFFORT_FIXED2, pcm, frames, first_block, final, out, out_capacity_bytes, result, frames_consumed);
}

int d2d_flac_encode_host_effort(uint32_t channels, uint32_t bit_depth, uint32_t effort, const void* pcm, size_t frames, uint32_t first_block,
                                int final, void* out, size_t out_capacity_bytes, d2d_flac_result* result, size_t* frames_consumed) {
    if (!effort_ok(effort)) return fail(D2D_ERR_PARAM, EFFORT_MESSAGE);
    if (!depth_ok(bit_depth)) return fail(D2D_ERR_PARAM, "FLAC holds 16, 20 or 24-bit integers (Invalid bit depth)");
    if (channels == 0 || channels > 8) return fail(D2D_ERR_PARAM, "FLAC holds 1 to 8 channels (Invalid channel count)");
    if (!result) return fail(D2D_ERR_PARAM, "null result record");
    const size_t blocks = block_count(frames, final);
    if ((uint64_t)first_block + blocks > (1ull << 31)) return fail(D2D_ERR_PARAM, "frame numbers are 31 bits: first_block + blocks exceeds 2^31");
    if (blocks && (!pcm || !out)) return fail(D2D_ERR_PARAM, "null pcm or out pointer");
    if (out_capacity_bytes < d2d_flac_bound_bytes(channels, bit_depth, frames, final)) return fail(D2D_ERR_CAPACITY, "out buffer below d2d_flac_bound_bytes");
    const uint32_t sb = sample_bytes(bit_depth);
    const uint8_t* p = (const uint8_t*)pcm;
    uint8_t* o = (uint8_t*)out;
    d2dhost::FlacFrameEnc enc;
    std::vector<int32_t> buf((size_t)BS * channels);
    d2d_flac_result r{0, 0, 0};
    for (size_t b = 0; b < blocks; ++b) {
        const uint32_t n = (uint32_t)std::min<size_t>(BS, frames - b * BS);
        const uint8_t* q = p + b * BS * channels * sb;
        for (size_t i = 0; i < (size_t)n * channels; ++i, q += sb) {      // as FlacSink::write unpacks them
            int32_t v = sb == 2 ? (int16_t)(q[0] | (q[1] << 8)) : (int32_t)((uint32_t)(q[0] | (q[1] << 8) | (q[2] << 16)) << 8) >> 8;
            if (bit_depth == 20) v >>= 4;
            buf[i] = v;
        }
        enc.encode(buf.data(), n, channels, bit_depth, first_block + (uint32_t)b, BS, effort);
        const uint32_t fs = (uint32_t)enc.out.size();
        memcpy(o + r.bytes_out, enc.out.data(), fs);
        r.bytes_out += fs;
        r.min_frame_bytes = b ? std::min(r.min_frame_bytes, fs) : fs;
        r.max_frame_bytes = std::max(r.max_frame_bytes, fs);
    }
    *result = r;
    if (frames_consumed) *frames_consumed = final ? frames : (frames / BS) * BS;
    return D2D_OK;
}

int d2d_flac_decode_host(uint32_t channels, uint32_t bit_depth, const void* frames, size_t bytes, uint32_t first_block,
                         void* pcm, size_t pcm_capacity_bytes, size_t* frames_out, d2d_flac_check* check) {
    if (!depth_ok(bit_depth)) return fail(D2D_ERR_PARAM, "FLAC holds 16, 20 or 24-bit integers (Invalid bit depth)");
    if (channels == 0 || channels > 8) return fail(D2D_ERR_PARAM, "FLAC holds 1 to 8 channels (Invalid channel count)");
    if (!check || !frames_out) return fail(D2D_ERR_PARAM, "null check record or frames_out");
    if (bytes && !frames) return fail(D2D_ERR_PARAM, "null frames pointer");
    const uint8_t* p = (const uint8_t*)frames;
    const uint16_t* tab = d2dhost::FlacFrameEnc::crc16_table();
    const size_t bound = frame_bound(channels, bit_depth, BS);
    const uint32_t sb = sample_bytes(bit_depth);
    std::vector<uint8_t> decoded;
    DecodeSig sig;
    d2d_flac_check c;
    clean_record(c);
    bool ended = false;                                               // a short block was the stream's last
    for (size_t off = 0, b = 0; off < bytes; ++b) {
        const uint64_t number = (uint64_t)first_block + b;
        d2dparse::Header h{0, 0, 0};
        uint32_t size = 0;
        uint32_t reason = ended || number >= (1ull << 31) ? (uint32_t)D2D_FLAC_BAD_HEADER
                        : d2dparse::parse_frame(p + off, (uint32_t)std::min(bytes - off, bound), false, d2dparse::Expect{channels, bit_depth, 0, (uint32_t)number}, tab, sig, h, &size);
        if (!reason && !sig.undo_stereo(h.assignment, h.n, bit_depth)) reason = D2D_FLAC_BAD_SAMPLES;
        count_block(c, (uint32_t)b, reason, h.n);
        if (reason) break;
        const size_t at = decoded.size();
        decoded.resize(at + (size_t)h.n * channels * sb);
        uint8_t* q = decoded.data() + at;
        for (uint32_t i = 0; i < h.n; ++i)
            for (uint32_t ch = 0; ch < channels; ++ch, q += sb) {
                const uint32_t v = (uint32_t)sig.x[ch][i] << (bit_depth == 20 ? 4 : 0);
                q[0] = (uint8_t)v; q[1] = (uint8_t)(v >> 8);
                if (sb == 3) q[2] = (uint8_t)(v >> 16);
            }
        ended = h.n != BS;
        off += size;
    }
    if (decoded.size() > pcm_capacity_bytes) return fail(D2D_ERR_CAPACITY, "pcm buffer below the decoded frames");
    if (!decoded.empty() && !pcm) return fail(D2D_ERR_PARAM, "null pcm pointer");
    if (!decoded.empty()) memcpy(pcm, decoded.data(), decoded.size());
    *frames_out = (size_t)c.samples_checked;
    *check = c;
    return D2D_OK;
}

int d2d_flac_verify_host(uint32_t channels, uint32_t bit_depth, const void* pcm, size_t frames, uint32_t first_block, int final,
                         const void* out, size_t bytes_out, const uint32_t* sizes, d2d_flac_check* check) {
    return d2d_flac_verify_host_method(channels, bit_depth, pcm, frames, first_block, final, out, bytes_out, sizes, check, D2D_FLAC_VERIFY_AUTO, nullptr);
}

int d2d_flac_verify_host_method(uint32_t channels, uint32_t bit_depth, const void* pcm, size_t frames, uint32_t first_block, int final,
                                const void* out, size_t bytes_out, const uint32_t* sizes, d2d_flac_check* check, uint32_t method,
                                d2d_flac_verify_stats* stats) {
    if (!verify_method_ok(method)) return fail(D2D_ERR_PARAM, VERIFY_METHOD_MESSAGE);
    if (!depth_ok(bit_depth)) return fail(D2D_ERR_PARAM, "FLAC holds 16, 20 or 24-bit integers (Invalid bit depth)");
    if (channels == 0 || channels > 8) return fail(D2D_ERR_PARAM, "FLAC holds 1 to 8 channels (Invalid channel count)");
    if (!check) return fail(D2D_ERR_PARAM, "null check record");
    const size_t blocks = block_count(frames, final);
    if ((uint64_t)first_block + blocks > (1ull << 31)) return fail(D2D_ERR_PARAM, "frame numbers are 31 bits: first_block + blocks exceeds 2^31");
    if (blocks && (!pcm || !out)) return fail(D2D_ERR_PARAM, "null pcm or out pointer");
    const uint8_t* o = (const uint8_t*)out;
    const uint16_t* tab = d2dhost::FlacFrameEnc::crc16_table();
    const uint32_t bound = (uint32_t)frame_bound(channels, bit_depth, BS);
    const size_t fb = (size_t)channels * sample_bytes(bit_depth);
    int32_t store[2 * d2dparse::MAX_LPC_ORDER];
    std::vector<int32_t> signal(method == D2D_FLAC_VERIFY_SERIAL ? 0 : BS);      // the cooperative rule's room for one coded signal
    d2d_flac_check c;
    clean_record(c);
    uint32_t fast = 0;
    uint64_t off = 0;
    bool lost = false;                                                // sizes == NULL: a walk that failed cannot find the later frames
    for (size_t b = 0; b < blocks; ++b) {
        const uint32_t n = (uint32_t)std::min<size_t>(BS, frames - b * BS);
        const d2dparse::Expect ex{channels, bit_depth, n, first_block + (uint32_t)b};
        const uint8_t* block_pcm = (const uint8_t*)pcm + b * BS * fb;
        uint32_t reason = D2D_FLAC_BAD_SIZE, size = 0;
        if (sizes) {
            size = sizes[b];
            if (d2dparse::size_ok(off, size, bytes_out, bound, b + 1 == blocks)) {
                if (method != D2D_FLAC_VERIFY_SERIAL && d2dexpect::accept_frame(o + off, size, ex, block_pcm, tab, signal.data())) { reason = D2D_FLAC_BAD_NONE; ++fast; }
                else reason = d2dparse::verify_frame(o + off, size, true, ex, block_pcm, tab, store, 1, nullptr);
            }
        } else if (!lost && off < bytes_out) {
            reason = d2dparse::verify_frame(o + off, (uint32_t)std::min<uint64_t>(bytes_out - off, bound), false, ex, block_pcm, tab, store, 1, &size);
            if (reason && reason != D2D_FLAC_BAD_SAMPLES) lost = true;       // (a frame that is not the PCM still has its end)
            else if (b + 1 == blocks && off + size != bytes_out) reason = D2D_FLAC_BAD_SIZE;
        }
        count_block(c, (uint32_t)b, reason, n);
        off += size;
    }
    *check = c;
    if (stats) *stats = d2d_flac_verify_stats{fast, (uint32_t)blocks - fast};
    return D2D_OK;
}

// ---- STREAMINFO's MD5: the CPU twins of d2d_flac_md5.hip ----

// the next n message bytes behind the record's tail; whole blocks go into h as they fill
static void md5_absorb(d2d_flac_md5_state& s, const uint8_t* p, size_t n) {
    s.bytes += n;
    uint32_t t = s.tail_bytes & 63u;
    while (n) {
        const uint32_t take = (uint32_t)std::min<size_t>(n, d2dmd5::BLOCK - t);
        memcpy(s.tail + t, p, take);
        t += take; p += take; n -= take;
        if (t == d2dmd5::BLOCK) {
            uint32_t m[16];
            for (int i = 0; i < 16; ++i) m[i] = d2dmd5::word_le(s.tail + 4 * i);
            d2dmd5::block(s.h, m);
            t = 0;
        }
    }
    s.tail_bytes = t;
}

void d2d_flac_md5_init_host(d2d_flac_md5_state* states, uint32_t n_files) {
    for (uint32_t f = 0; states && f < n_files; ++f) {
        memset(&states[f], 0, sizeof(states[f]));
        states[f].h[0] = d2dmd5::H0; states[f].h[1] = d2dmd5::H1; states[f].h[2] = d2dmd5::H2; states[f].h[3] = d2dmd5::H3;
    }
}

int d2d_flac_md5_update_host(uint32_t channels, uint32_t bit_depth, const void* pcm, size_t frames, d2d_flac_md5_state* state) {
    if (!depth_ok(bit_depth)) return fail(D2D_ERR_PARAM, "FLAC holds 16, 20 or 24-bit integers (Invalid bit depth)");
    if (channels == 0 || channels > 8) return fail(D2D_ERR_PARAM, "FLAC holds 1 to 8 channels (Invalid channel count)");
    if (!state) return fail(D2D_ERR_PARAM, "null MD5 state");
    if (frames && !pcm) return fail(D2D_ERR_PARAM, "null pcm pointer");
    if (frames > MD5_MAX_FRAMES) return fail(D2D_ERR_PARAM, "more frames than a byte count of 64 bits holds");
    if (!frames) return D2D_OK;
    const uint8_t* p = (const uint8_t*)pcm;
    const size_t n = frames * channels * sample_bytes(bit_depth);
    if (bit_depth != 20) md5_absorb(*state, p, n);
    else {
        uint8_t buf[3 * 1024];                                        // the 20-bit rule, 1024 samples at a time
        for (size_t at = 0; at < n;) {
            const size_t take = std::min(n - at, sizeof(buf));
            for (size_t i = 0; i < take; i += 3) {
                const uint32_t v = d2dmd5::sample20((uint32_t)p[at + i] | ((uint32_t)p[at + i + 1] << 8) | ((uint32_t)p[at + i + 2] << 16));
                buf[i] = (uint8_t)v; buf[i + 1] = (uint8_t)(v >> 8); buf[i + 2] = (uint8_t)(v >> 16);
            }
            md5_absorb(*state, buf, take);
            at += take;
        }
    }
    memset(state->tail + state->tail_bytes, 0, d2dmd5::BLOCK - state->tail_bytes);      // (as the kernel leaves the record)
    return D2D_OK;
}

int d2d_flac_md5_final_host(const d2d_flac_md5_state* state, uint8_t digest[16]) {
    if (!state || !digest) return fail(D2D_ERR_PARAM, "null MD5 state or digest");
    d2dmd5::finish(state->h, state->bytes, state->tail, digest);
    return D2D_OK;
}

}  // extern "C"
