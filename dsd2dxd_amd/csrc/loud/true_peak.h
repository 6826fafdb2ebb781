// true_peak.h -- the true-peak cell (include/dsd2dxd_amd.h, "Loudness where the PCM is") as the host twin and the GPU kernel must agree
// on it bit for bit.  One copy, plain C++, compiled for the host (g++) and for the device (hipcc); no inline assembly, no libm.  The
// sample values are loud_meter.h's d2dloud::sample(), exact for all four depths.
//
// THE DEFINITION.  The signal is oversampled four times, at every rate, by four phases of twelve taps whose coefficients are INTEGERS
// over 8192 (13 fractional bits) -- the table below is this project's definition:
//
//     phase 0:   14   90 -161  272  -487 1125 7964  -838  390 -218  122  -68          (sum 8205, sum of magnitudes 11749)
//     phase 1: -239  240 -424  730 -1364 3810 6388 -1641  832 -477  271 -155          (sum 7971, sum of magnitudes 16571)
//     phase 2: phase 1 reversed
//     phase 3: phase 0 reversed
//
// For input frame n >= 0 of the stream, channel c and phase p:  y_p(n) = sum over k = 0 .. 11 of C[p][k] * x_c(n - k), with x = 0 before
// frame 0, accumulated in f64 from 0.0 in the order k = 0, 1, .. 11; the value reported is |y| * 2^-13.
//
// WHY THE DECOMPOSITION IS FREE.  Every product is exact in f64: an integer of at most 14 bits times a value of at most 24 significant
// bits.  So fusing a multiplication into the addition behind it, or not, cannot change a bit, and this header needs no contraction
// switch.  For 16/20/24-bit input every partial sum is exact as well (|y| < 2^38 in units of the input's last bit): any order would do.
// Only float input rounds, and only in the twelve additions, whose order is fixed above.  A y_p(n) depends on twelve input frames and on
// nothing else, so host and device agree bit for bit however the frames are spread over lanes, tiles, workgroups or calls.
//
// THE CELL of sub-block j (S = rate / 10 frames), channel c is the largest |y_p(n)| * 2^-13 over n in [j S, (j + 1) S) -- to the
// stream's end for the partial row -- and p = 0 .. 3.  Two choices to know:
//   * an output belongs to the sub-block of its index n: the filter is causal and its delay of about six frames is NOT compensated;
//   * the eleven outputs behind the last frame of a stream (the filter's tail) are DROPPED.
// Because of the second, a stream's last few samples may be seen by fewer taps than their neighbours, and the figure a meter reports is
// max(sample peak, largest true-peak cell) (d2d_loud_true_peak), never below the sample peak.
//
// Input is finite; non-finite float samples give an unspecified value.
#pragma once
#include "loud_meter.h"

namespace d2dtp {

constexpr uint32_t TAPS = 12, PHASES = 4;
constexpr uint32_t HISTORY = TAPS - 1;                            // frames in front of an output's own that it reads
constexpr double SCALE = 1.0 / 8192.0;                            // 2^-13

// the table as numbers, for code that wants to index it (tools, tests); the arithmetic below spells the same integers out
constexpr int32_t COEF[PHASES][TAPS] = {
    {14, 90, -161, 272, -487, 1125, 7964, -838, 390, -218, 122, -68},
    {-239, 240, -424, 730, -1364, 3810, 6388, -1641, 832, -477, 271, -155},
    {-155, 271, -477, 832, -1641, 6388, 3810, -1364, 730, -424, 240, -239},
    {-68, 122, -218, 390, -838, 7964, 1125, -487, 272, -161, 90, 14},
};

// where the history of sub-block j begins, in frames: max(0, j S - 11)
D2D_LOUD_HD uint64_t history_start(uint64_t j, uint64_t S) { return j * S > HISTORY ? j * S - HISTORY : 0; }

// The largest |y_p(n)|, p = 0 .. 3, of one frame n, NOT yet scaled by 2^-13 (the scaling is exact and monotonic: it is applied once,
// to the maximum).  `x` points at x(n) in a run of samples in time order: x[-k] is x(n - k), k = 0 .. 11, zeros before frame 0.
D2D_LOUD_HD double frame_peak(const double* x) {
    double y0 = 0.0, y1 = 0.0, y2 = 0.0, y3 = 0.0;
    // k: the tap; a, b: phase 0's and phase 1's coefficient there; c, d: phase 2's and phase 3's (b and a read from the other end)
    // (the device asks for the fused form by name, since its units are built with -ffp-contract=off for loud_meter.h: v_fma_f64, half
    // the instructions; the product being exact, it is the same double as the host's multiplication and addition)
#if defined(__HIP_DEVICE_COMPILE__)
#define D2D_TP_MAC(y, a, v) y = __builtin_fma((double)(a), v, y);
#else
#define D2D_TP_MAC(y, a, v) y = y + (double)(a) * v;
#endif
#define D2D_TP_TAP(k, a, b, c, d) \
    { const double v = x[-(k)]; D2D_TP_MAC(y0, a, v) D2D_TP_MAC(y1, b, v) D2D_TP_MAC(y2, c, v) D2D_TP_MAC(y3, d, v) }
    D2D_TP_TAP(0, 14, -239, -155, -68)
    D2D_TP_TAP(1, 90, 240, 271, 122)
    D2D_TP_TAP(2, -161, -424, -477, -218)
    D2D_TP_TAP(3, 272, 730, 832, 390)
    D2D_TP_TAP(4, -487, -1364, -1641, -838)
    D2D_TP_TAP(5, 1125, 3810, 6388, 7964)
    D2D_TP_TAP(6, 7964, 6388, 3810, 1125)
    D2D_TP_TAP(7, -838, -1641, -1364, -487)
    D2D_TP_TAP(8, 390, 832, 730, 272)
    D2D_TP_TAP(9, -218, -477, -424, -161)
    D2D_TP_TAP(10, 122, 271, 240, 90)
    D2D_TP_TAP(11, -68, -155, -239, 14)
#undef D2D_TP_TAP
#undef D2D_TP_MAC
    const double a0 = y0 < 0.0 ? -y0 : y0, a1 = y1 < 0.0 ? -y1 : y1, a2 = y2 < 0.0 ? -y2 : y2, a3 = y3 < 0.0 ? -y3 : y3;
    const double m01 = a0 > a1 ? a0 : a1, m23 = a2 > a3 ? a2 : a3;
    return m01 > m23 ? m01 : m23;
}

}  // namespace d2dtp
