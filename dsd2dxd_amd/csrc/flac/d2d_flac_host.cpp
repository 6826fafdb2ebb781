// d2d_flac_host.cpp -- the host half of the FLAC entry points: sizes, the error slot and d2d_flac_encode_host, which is the sink's
// own frame encoder (flac_frame_enc.h) behind the C ABI.  No HIP: tools and tests build this file with g++ alone.
#include <string.h>

#include <algorithm>
#include <vector>

#include "d2d_flac_internal.h"
#include "flac_frame_enc.h"

namespace d2dflac {

static thread_local std::string g_flac_error;
int fail(int code, const std::string& message) { g_flac_error = message; return code; }

}  // namespace d2dflac

using namespace d2dflac;

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

}  // extern "C"
