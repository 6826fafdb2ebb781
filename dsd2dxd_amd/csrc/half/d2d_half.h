// d2d_half.h -- the exact 2:1 decimator between the FIR sums and the requantiser, once: the table, the integer
// arithmetic of one output and the frame count.  One source for the device kernel (half/d2d_half.hip), its CPU twin
// (half/d2d_half_host.cpp) and tools/half_fuzz.cpp.  No HIP include, like d2d_sample.h and mix/d2d_mix.h: the functions compile for the
// device under hipcc and for the host under any C++17 compiler.  Meant for -ffp-contract=off.
//
//   x[i]  a channel's exact integer FIR sum at index i of the 88.2 / 96 kHz sequence, scale 2^-S (the scratch line the FIR kernels'
//         to_scratch form writes); x[i] = 0 for i < 0
//   v[k] = sum_j q[j] x[2k - j]            an exact 64-bit integer: |x| < 2^31 and sum |q| < 2^28 keep |v| < 2^59
//   w[k] = (v[k] + 2^(T-1)) >> T           arithmetic shift: back on the scratch grid, ties towards +infinity; |w| < 2^33
//   y[k] = (double)w[k] * 2^-S             exact, and from there the arithmetic of every other path (d2d_sample.h) at output index k
//
// Output k exists as soon as x[2k] does: after n sums a stream has produced (n + 1) >> 1 frames.  The filter's delay of (NT - 1) / 2
// sums is not compensated.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../../filters/half_table.inc"
#include "../d2d_internal.h"
#include "../d2d_sample.h"
#include "../mix/d2d_mix.h"        // mix_sample_bits, mix_epilogue: the requantiser from y on is the mix pass's

namespace d2d {

constexpr int HALF_NT = D2D_HALF_NT, HALF_T = D2D_HALF_T;
constexpr uint32_t HALF_HIST = HALF_NT - 1;            // sums carried in front of a line
constexpr uint32_t HALF_MAX_CHANNELS = 64;             // d2d_create's limit
static_assert(HALF_NT % 2 == 1 && HALF_NT <= 511 && HALF_T >= 1 && HALF_T <= 28, "the half table's shape");

// frames a stream has produced once it holds n sums
D2D_HD uint64_t half_frames_after(uint64_t n) { return (n + 1) >> 1; }

// v[k] from the line: xk points at x[2k]; the NT - 1 sums in front of it are read
D2D_HD int64_t half_sum(const int32_t* q, const int32_t* xk) {
    int64_t v = 0;
    for (int j = 0; j < HALF_NT; ++j) v += (int64_t)q[j] * (int64_t)xk[-j];
    return v;
}
// w[k]: round to the scratch grid, ties towards +infinity
D2D_HD int64_t half_round(int64_t v) { return (v + ((int64_t)1 << (HALF_T - 1))) >> HALF_T; }
D2D_HD double half_value(int64_t w, double two_to_minus_s) { return (double)w * two_to_minus_s; }

}  // namespace d2d
