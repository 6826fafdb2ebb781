// d2d_mix_host.cpp -- the host half of the channel matrix: d2d_mix_frames_host, the CPU twin of d2d_mix_kernel (the same header, the same
// order of operations), d2d_mix_preset and the "--mix" text parser the CLI and the host driver share.  No HIP: tools/mix_fuzz.cpp builds
// from it with g++ alone.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../../include/dsd2dxd_amd.h"
#include "d2d_mix.h"
#include "d2d_mix_text.h"

using namespace d2d;

namespace {
thread_local std::string g_mix_error;
int fail(int code, const char* m) { g_mix_error = m; return code; }
}  // namespace

namespace d2d {

// "g,g,..;g,g,.." -- rows separated by ';', decimal gains by ',', every row as long as the first; gains are rounded to Q15 half away from zero.
// The bounds are mix_check's; the column count is the caller's to compare with the stream's.
bool parse_mix_text(const char* text, std::vector<int32_t>& coef, uint32_t& rows, uint32_t& cols, std::string& err) {
    coef.clear(); rows = cols = 0;
    if (!text) { err = "Invalid mix: empty"; return false; }
    const char* p = text;
    uint32_t in_row = 0;
    for (;;) {
        while (*p == ' ' || *p == '\t') ++p;
        char* end = nullptr;
        const double g = strtod(p, &end);
        if (end == p || !isfinite(g)) { err = "Invalid mix: expected a decimal gain"; return false; }
        if (fabs(g) > 4.0) { err = "Invalid mix: a coefficient is above 4.0 (2^17 in Q15)"; return false; }
        coef.push_back((int32_t)(g < 0 ? -floor(-g * 32768.0 + 0.5) : floor(g * 32768.0 + 0.5)));
        ++in_row;
        if (coef.size() > (size_t)MIX_MAX_CHANNELS * MIX_MAX_CHANNELS) { err = "Invalid mix: too many coefficients"; return false; }
        p = end;
        while (*p == ' ' || *p == '\t') ++p;
        if (*p == ',') { ++p; continue; }
        if (*p == ';' || *p == '\0') {
            if (rows == 0) cols = in_row;
            else if (in_row != cols) { err = "Invalid mix: every row needs the same number of gains"; return false; }
            ++rows; in_row = 0;
            if (*p == '\0') break;
            ++p;
            continue;
        }
        err = "Invalid mix: unexpected character (rows are separated by ';', gains by ',')";
        return false;
    }
    if (const char* why = mix_check(cols, rows, coef.data())) { err = why; return false; }
    return true;
}

}  // namespace d2d

extern "C" {

const char* d2d_mix_error(void) { return g_mix_error.c_str(); }

int d2d_mix_preset(uint32_t in_channels, uint32_t layout, uint32_t target, int32_t* coef, uint32_t* out_channels) {
    if (!coef || !out_channels) return fail(D2D_ERR_PARAM, "null argument");
    if (const char* why = mix_preset(in_channels, layout, target, coef, out_channels)) return fail(D2D_ERR_PARAM, why);
    return D2D_OK;
}

int d2d_mix_frames_host(const int32_t* sums, size_t stride, size_t frames, uint32_t in_channels, int32_t scale_bits, const d2d_mix* mix,
                        uint32_t bit_depth, uint32_t dither, double level_db, uint64_t seed, uint64_t first_index,
                        void* pcm, size_t pcm_capacity_bytes, double* peaks) {
    if (!mix || mix->struct_size != sizeof(d2d_mix)) return fail(D2D_ERR_PARAM, "d2d_mix.struct_size mismatch");
    if (const char* why = mix_check(in_channels, mix->out_channels, mix->coef)) return fail(D2D_ERR_PARAM, why);
    if (bit_depth != 16 && bit_depth != 20 && bit_depth != 24 && bit_depth != 32) return fail(D2D_ERR_PARAM, "Invalid bit depth; must be 16, 20, 24 or 32");
    if (dither != 'T' && dither != 'R' && dither != 'F' && dither != 'X') return fail(D2D_ERR_PARAM, "Invalid dither type; must be T, R, F, or X");
    if (!isfinite(level_db)) return fail(D2D_ERR_PARAM, "Invalid level");
    if (scale_bits < 0 || scale_bits > 40) return fail(D2D_ERR_PARAM, "Invalid scale");
    if (frames && (!sums || stride < frames)) return fail(D2D_ERR_PARAM, "the sums do not hold that many frames");
    const uint32_t C = in_channels, Co = mix->out_channels;
    const Epilogue epi = mix_epilogue(bit_depth, dither, level_db, seed, Co);
    const size_t sb = epi.sample_bytes, fb = sb * Co;
    if (frames > pcm_capacity_bytes / fb) return fail(D2D_ERR_CAPACITY, "pcm buffer too small");
    if (frames && !pcm) return fail(D2D_ERR_PARAM, "null pcm pointer");
    const double ys = ldexp(1.0, -(scale_bits + MIX_Q));
    uint64_t keys[MIX_MAX_CHANNELS];
    for (uint32_t o = 0; o < Co; ++o) keys[o] = dither_key64(seed, o);
    int32_t x[MIX_MAX_CHANNELS];
    uint8_t* out = (uint8_t*)pcm;
    for (size_t n = 0; n < frames; ++n) {
        for (uint32_t c = 0; c < C; ++c) x[c] = sums[(size_t)c * stride + n];
        for (uint32_t o = 0; o < Co; ++o) {
            const double y = mix_value(mix_sum(mix->coef + (size_t)o * C, x, C), ys);
            const uint32_t w = mix_sample_bits(epi, y, dither_word_at(keys[o], first_index + n));
            memcpy(out + n * fb + o * sb, &w, sb);           // (little-endian hosts: the low sample_bytes bytes)
            if (peaks) peaks[o] = fmax(peaks[o], fabs(y * epi.gain));
        }
    }
    return D2D_OK;
}

}  // extern "C"
