// loud_meter.h -- the loudness cell (include/dsd2dxd_amd.h, "Loudness where the PCM is") as the host twin and the GPU kernel must agree
// on it bit for bit: the sample conversions, the two K-weighting biquads, and the sums of one (sub-block, channel) unit.  One copy, plain
// C++, compiled for the host (g++) and for the device (hipcc); no inline assembly, no libm.  Multiplications and additions only, and
// none of them may fuse: every unit that includes this header is built with -ffp-contract=off, and the routines say so again with the
// pragma.  THE ORDER OF OPERATIONS WRITTEN HERE IS THE DEFINITION.
//
// This is ITU-R BS.1770 / EBU R128 with one deliberate change: the filter of sub-block j (S = rate / 10 frames, 100 ms) starts from rest
// at frame max(0, j - 2) * S, two sub-blocks of pre-roll, instead of running through the stream.  The high-pass has decayed by about
// e^-47 after 200 ms (measured: sub-block energies within 1.1e-13 relative of an uninterrupted pass), and every (file, sub-block,
// channel) becomes independent work whose result does not depend on where a stream is cut into calls.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define D2D_LOUD_HD __host__ __device__ __forceinline__
#else
#define D2D_LOUD_HD inline
#endif
#if defined(__clang__)
#define D2D_LOUD_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define D2D_LOUD_NO_CONTRACT                                      // g++: -ffp-contract=off on the command line (csrc/Makefile)
#endif

namespace d2dloud {

constexpr uint32_t PREROLL = 2;                                   // sub-blocks the filter runs before the one it measures
constexpr uint32_t RATE_MIN = 8000, RATE_MAX = 1411200;

inline bool depth_ok(uint32_t d) { return d == 16 || d == 20 || d == 24 || d == 32; }
inline bool rate_ok(uint32_t r) { return r >= RATE_MIN && r <= RATE_MAX && r % 10 == 0; }
D2D_LOUD_HD uint32_t sample_bytes(uint32_t depth) { return depth == 16 ? 2u : depth == 32 ? 4u : 3u; }

// The ten doubles of d2d_loud_coefficients, in this order.  Both stages are transposed direct form II with a0 = 1.
struct Coef {
    double sb0, sb1, sb2, sa1, sa2;                               // the shelf
    double hb0, hb1, hb2, ha1, ha2;                               // the high-pass (b = 1, -2, 1)
};

// a sample from its little-endian bytes, `raw` in the low bits: exact in all three cases
//   16 bits: v / 2^15;  20 and 24 bits: the 3-byte container value / 2^23;  32 bits: the float, widened
D2D_LOUD_HD double sample(uint32_t raw, uint32_t depth) {
    if (depth == 16) return (double)(int32_t)(int16_t)(uint16_t)raw * (1.0 / 32768.0);
    if (depth == 32) {
        union { uint32_t u; float f; } v;
        v.u = raw;
        return (double)v.f;
    }
    return (double)((int32_t)(raw << 8) >> 8) * (1.0 / 8388608.0);
}

// the state of one unit: both filters at rest, nothing summed
struct Unit {
    double s1 = 0.0, s2 = 0.0;                                    // the shelf's two delays
    double h1 = 0.0, h2 = 0.0;                                    // the high-pass's
    double energy = 0.0, peak = 0.0;
};

// one frame through both filters; returns y
D2D_LOUD_HD double filter(Unit& u, const Coef& k, double x) {
    D2D_LOUD_NO_CONTRACT
    const double v = k.sb0 * x + u.s1;
    const double p1 = k.sb1 * x, q1 = k.sa1 * v;
    u.s1 = (p1 - q1) + u.s2;
    const double p2 = k.sb2 * x, q2 = k.sa2 * v;
    u.s2 = p2 - q2;
    const double y = k.hb0 * v + u.h1;
    const double r1 = k.hb1 * v, t1 = k.ha1 * y;
    u.h1 = (r1 - t1) + u.h2;
    const double r2 = k.hb2 * v, t2 = k.ha2 * y;
    u.h2 = r2 - t2;
    return y;
}

// a frame of the pre-roll: filtered, not counted
D2D_LOUD_HD void preroll(Unit& u, const Coef& k, double x) { (void)filter(u, k, x); }

// a frame of the sub-block itself: the product is rounded, then added; the peak is of |x|
D2D_LOUD_HD void measure(Unit& u, const Coef& k, double x) {
    D2D_LOUD_NO_CONTRACT
    const double y = filter(u, k, x);
    const double yy = y * y;
    u.energy = u.energy + yy;
    const double ax = x < 0.0 ? -x : x;
    if (ax > u.peak) u.peak = ax;
}

// where the filter of sub-block j starts, in sub-blocks
D2D_LOUD_HD uint64_t start_subblock(uint64_t j) { return j > PREROLL ? j - PREROLL : 0; }

}  // namespace d2dloud
