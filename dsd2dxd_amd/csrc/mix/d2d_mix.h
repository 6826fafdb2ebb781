// d2d_mix.h -- the channel matrix between the FIR sums and the requantiser, once: the bounds d2d_create_mix checks,
// the per-frame arithmetic of the mix pass and the fold-down presets.  One source for the device kernel (mix/d2d_mix.hip), its CPU twin
// (mix/d2d_mix_host.cpp) and tools/mix_fuzz.cpp.  No HIP include, like d2d_sample.h: the functions compile for the device under hipcc and
// for the host under any C++17 compiler.  Meant for -ffp-contract=off.
//
//   x_c   the exact integer FIR sum of input channel c at one output index, scale 2^-S (the scratch line the FIR kernels' to_scratch form writes)
//   v_o = sum_c m[o][c] x_c      an exact 64-bit integer: |m| <= 2^17, sum_c |m[o][c]| <= 2^21 and |x| < 2^31 keep |v| < 2^52
//   y_o = (double)v_o * 2^-(S+15)   exact, and from there the arithmetic of every other path (d2d_sample.h) on OUTPUT channel o
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../d2d_internal.h"
#include "../d2d_sample.h"

namespace d2d {

constexpr int MIX_Q = 15;                              // coefficients are Q15: gain = m / 32768
constexpr int32_t MIX_UNITY = 1 << MIX_Q;
constexpr int32_t MIX_COEF_MAX = 1 << 17;              // |m| <= 4.0
constexpr int64_t MIX_ROW_MAX = (int64_t)1 << 21;      // sum_c |m[o][c]| <= 64.0
constexpr uint32_t MIX_MAX_CHANNELS = 64;              // d2d_create's limit

// the bounds of a mix of `rows` x `cols` coefficients; nullptr when they hold, else the reason
inline const char* mix_check(uint32_t cols, uint32_t rows, const int32_t* m) {
    if (cols < 1 || cols > MIX_MAX_CHANNELS) return "Invalid channel count";
    if (rows < 1 || rows > cols) return "Invalid mix: out_channels must be between 1 and the channel count";
    if (!m) return "Invalid mix: null coefficients";
    for (uint32_t o = 0; o < rows; ++o) {
        int64_t sum = 0;
        for (uint32_t c = 0; c < cols; ++c) {
            const int64_t a = m[(size_t)o * cols + c] < 0 ? -(int64_t)m[(size_t)o * cols + c] : (int64_t)m[(size_t)o * cols + c];
            if (a > MIX_COEF_MAX) return "Invalid mix: a coefficient is above 4.0 (2^17 in Q15)";
            sum += a;
        }
        if (sum > MIX_ROW_MAX) return "Invalid mix: a row's absolute coefficients sum to more than 64.0 (2^21 in Q15)";
    }
    return nullptr;
}

// one output channel of one frame: the exact integer, and its value (sbits = S + 15)
D2D_HD int64_t mix_sum(const int32_t* row, const int32_t* x, uint32_t cols) {
    int64_t v = 0;
    for (uint32_t c = 0; c < cols; ++c) v += (int64_t)row[c] * (int64_t)x[c];
    return v;
}
D2D_HD double mix_value(int64_t v, double two_to_minus_sbits) { return (double)v * two_to_minus_sbits; }

// The epilogue of d2d_device.h's emit_sample from the finished steps of d2d_sample.h: the sample of y as it sits in its container
// (16 / 24 low bits, 20-bit samples shifted into 24, or the float's bits).  The same value for every y and word as quantise_int /
// quantise_f32 there (tests/test_sample_arithmetic.py holds the two forms of the integer depths together).
D2D_HD uint32_t mix_sample_bits(const Epilogue& ep, double y, uint32_t word) {
    if (ep.bits == 32) {
        double x = y * ep.gain;
        if (ep.dither == 'F') x = dither_float(x, word);
        return f32_bits((float)x);
    }
    const double x = y * ep.scale;
    double d = 0.0;
    if (ep.dither == 'T') d = dither_f64<DITHER_TRI>(dither_term<DITHER_TRI>(word));
    else if (ep.dither == 'R') d = dither_f64<DITHER_RECT>(dither_term<DITHER_RECT>(word));
    const int32_t iv = round_clip(x + d, (double)(1u << (ep.bits - 1)));
    return (uint32_t)(ep.bits == 20 ? iv * 16 : iv);
}

// ---- the fold-down presets (include/dsd2dxd_amd.h: d2d_mix_preset) -------------------------------------------------------------------
// Rows Lo, Ro in Q15, columns in container order.  Every row sums to at most 32768, so the fold cannot clip where no single channel
// could; the LFE column is zero.  1/sqrt(2) of a row's front gain goes to the centre and the surrounds.
enum MixLayout : uint32_t {
    MIX_LAYOUT_AUTO = 0,        // by channel count: 2 stereo, 3 L R C, 4 quad, 5 5.0, 6 5.1
    MIX_LAYOUT_STEREO = 2,      // FL FR
    MIX_LAYOUT_LRC = 3,         // FL FR C
    MIX_LAYOUT_QUAD = 4,        // FL FR BL BR
    MIX_LAYOUT_5_0 = 5,         // FL FR C BL BR
    MIX_LAYOUT_5_1 = 6,         // FL FR C LFE BL BR
    MIX_LAYOUT_LRC_LFE = 7,     // FL FR C LFE
};
struct MixPreset { uint32_t layout, channels; int32_t lo[6], ro[6]; };
constexpr MixPreset MIX_PRESETS[] = {
    {MIX_LAYOUT_STEREO, 2, {32768, 0}, {0, 32768}},
    {MIX_LAYOUT_LRC, 3, {19195, 0, 13573}, {0, 19195, 13573}},
    {MIX_LAYOUT_QUAD, 4, {19195, 0, 13573, 0}, {0, 19195, 0, 13573}},
    {MIX_LAYOUT_5_0, 5, {13573, 0, 9597, 9597, 0}, {0, 13573, 9597, 0, 9597}},
    {MIX_LAYOUT_5_1, 6, {13573, 0, 9597, 0, 9597, 0}, {0, 13573, 9597, 0, 0, 9597}},
    {MIX_LAYOUT_LRC_LFE, 4, {19195, 0, 13573, 0}, {0, 19195, 13573, 0}},
};

// coef: rows x in_channels; target 2: Lo, Ro; target 1: floor((Lo + Ro) / 2) per column.  Stereo has no stereo fold.  nullptr, or the reason
inline const char* mix_preset(uint32_t in_channels, uint32_t layout, uint32_t target, int32_t* coef, uint32_t* rows) {
    if (target != 1 && target != 2) return "Invalid downmix target; must be 1 (mono) or 2 (stereo)";
    if (layout == MIX_LAYOUT_AUTO) layout = in_channels >= 2 && in_channels <= 6 ? in_channels : 0xFFFFFFFFu;
    for (const MixPreset& p : MIX_PRESETS) {
        if (p.layout != layout) continue;
        if (p.channels != in_channels) return "Invalid downmix: the layout does not have this many channels";
        if (layout == MIX_LAYOUT_STEREO && target == 2) return "Invalid downmix: the stream is stereo already";
        for (uint32_t c = 0; c < in_channels; ++c) {
            if (target == 2) { coef[c] = p.lo[c]; coef[in_channels + c] = p.ro[c]; }
            else coef[c] = (p.lo[c] + p.ro[c]) >> 1;
        }
        *rows = target;
        return nullptr;
    }
    return "Invalid downmix: no preset for this channel layout (use an explicit mix)";
}

// the epilogue of a depth, dither and level, as d2d_route.cpp's epilogue_of makes it (host only)
inline Epilogue mix_epilogue(uint32_t bit_depth, uint32_t dither, double level_db, uint64_t seed, uint32_t out_channels) {
    Epilogue epi{};
    epi.gain = pow(10.0, level_db / 20.0);
    epi.scale = bit_depth == 32 ? epi.gain : ldexp(epi.gain, (int)bit_depth - 1);
    epi.seed = seed;
    epi.bits = bit_depth;
    epi.dither = dither;
    epi.sample_bytes = bit_depth == 16 ? 2 : (bit_depth == 32 ? 4 : 3);
    epi.channels = out_channels;
    return epi;
}

}  // namespace d2d
