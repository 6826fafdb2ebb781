// d2d_half_host.cpp -- the host half of the 2:1 decimator: d2d_half_frames_host, the CPU twin of d2d_half_kernel (the same header, the
// same integers), the checks both entry points share and d2d_half_taps.  No HIP: tools/half_fuzz.cpp builds from it with g++ alone.
#include <math.h>
#include <string.h>

#include <string>

#include "../../../include/dsd2dxd_amd.h"
#include "d2d_half.h"
#include "d2d_half_internal.h"

using namespace d2d;

namespace {
thread_local std::string g_half_error;
}  // namespace

namespace d2d {

int half_fail(int code, const char* m) { g_half_error = m; return code; }

// what both entry points check before anything is written; fills every frames_out
int half_check_jobs(d2d_half_job* jobs, uint32_t n_jobs, uint32_t channels, int32_t scale_bits, uint32_t bit_depth, uint32_t dither, double level_db) {
    if (n_jobs && !jobs) return half_fail(D2D_ERR_PARAM, "null argument");
    if (channels < 1 || channels > HALF_MAX_CHANNELS) return half_fail(D2D_ERR_PARAM, "Invalid channel count");
    if (bit_depth != 16 && bit_depth != 20 && bit_depth != 24 && bit_depth != 32) return half_fail(D2D_ERR_PARAM, "Invalid bit depth; must be 16, 20, 24 or 32");
    if (dither != 'T' && dither != 'R' && dither != 'F' && dither != 'X') return half_fail(D2D_ERR_PARAM, "Invalid dither type; must be T, R, F, or X");
    if (!isfinite(level_db)) return half_fail(D2D_ERR_PARAM, "Invalid level");
    if (scale_bits < 0 || scale_bits > 40) return half_fail(D2D_ERR_PARAM, "Invalid scale");
    const size_t fb = (size_t)(bit_depth == 16 ? 2 : bit_depth == 32 ? 4 : 3) * channels;
    for (uint32_t f = 0; f < n_jobs; ++f) {
        const d2d_half_job& j = jobs[f];
        if (j.n >= ((size_t)1 << 31)) return half_fail(D2D_ERR_PARAM, "n must be below 2^31 per job");
        if (j.first_index + j.n < j.first_index) return half_fail(D2D_ERR_PARAM, "first_index + n overflows");
        if (j.n && (!j.sums || j.stride < j.n + HALF_HIST)) return half_fail(D2D_ERR_PARAM, "the sums do not hold the history and that many new ones");
        const uint64_t frames = half_frames_after(j.first_index + j.n) - half_frames_after(j.first_index);
        if (frames > j.pcm_capacity_bytes / fb) return half_fail(D2D_ERR_CAPACITY, "pcm buffer too small");
        if (frames && !j.pcm) return half_fail(D2D_ERR_PARAM, "null pcm pointer");
    }
    for (uint32_t f = 0; f < n_jobs; ++f)
        jobs[f].frames_out = (size_t)(half_frames_after(jobs[f].first_index + jobs[f].n) - half_frames_after(jobs[f].first_index));
    return D2D_OK;
}

}  // namespace d2d

extern "C" {

const char* d2d_half_error(void) { return g_half_error.c_str(); }

int d2d_half_taps(uint32_t* nt, uint32_t* t, int32_t* taps, size_t capacity) {
    if (!nt || !t) return half_fail(D2D_ERR_PARAM, "null argument");
    *nt = (uint32_t)HALF_NT; *t = (uint32_t)HALF_T;
    if (taps) {
        if (capacity < (size_t)HALF_NT) return half_fail(D2D_ERR_CAPACITY, "tap buffer too small");
        memcpy(taps, D2D_HALF_TAPS, sizeof(int32_t) * HALF_NT);
    }
    return D2D_OK;
}

int d2d_half_frames_host(d2d_half_job* jobs, uint32_t n_jobs, uint32_t channels, int32_t scale_bits,
                         uint32_t bit_depth, uint32_t dither, double level_db, uint64_t seed) {
    if (int rc = half_check_jobs(jobs, n_jobs, channels, scale_bits, bit_depth, dither, level_db)) return rc;
    const Epilogue epi = mix_epilogue(bit_depth, dither, level_db, seed, channels);
    const size_t sb = epi.sample_bytes, fb = sb * channels;
    const double ys = ldexp(1.0, -scale_bits);
    for (uint32_t f = 0; f < n_jobs; ++f) {
        const d2d_half_job& j = jobs[f];
        const uint64_t k0 = half_frames_after(j.first_index);
        uint8_t* out = (uint8_t*)j.pcm;
        for (uint32_t c = 0; c < channels; ++c) {
            const uint64_t key = dither_key64(seed, c);
            const int32_t* x = j.sums + (size_t)c * j.stride + HALF_HIST;      // x[i]: the new sum of absolute index first_index + i
            for (size_t t = 0; t < j.frames_out; ++t) {
                const uint64_t k = k0 + t;
                const double y = half_value(half_round(half_sum(D2D_HALF_TAPS, x + (ptrdiff_t)(2 * k - j.first_index))), ys);
                const uint32_t w = mix_sample_bits(epi, y, dither_word_at(key, k));
                memcpy(out + t * fb + c * sb, &w, sb);           // (little-endian hosts: the low sample_bytes bytes)
                if (j.peaks) j.peaks[c] = fmax(j.peaks[c], fabs(y * epi.gain));
            }
        }
    }
    return D2D_OK;
}

}  // extern "C"
