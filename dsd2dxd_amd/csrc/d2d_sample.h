// d2d_sample.h -- the per-sample arithmetic contract, once: the dither generator, the dither terms, the f64
// requantiser, Airwindows "Dither Float", the all-integer requantiser and the limb recombination of the int8 matrix kernels.
// Every kernel's epilogue is a composition of these (d2d_device.h holds the compositions and the variants that need inline asm).
// No HIP include: the functions compile for the device under hipcc and for the host under any C++17 compiler
// (tools/sample_probe.cpp, tests/test_sample_arithmetic.py).  Meant for -ffp-contract=off: every f64 operation below is the single
// IEEE operation written, and an fma is an fma.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define D2D_HD __host__ __device__ __forceinline__
#else
#define D2D_HD inline
#endif

namespace d2d {

// dither kinds of the integer depths, as Mfma2Args::dkind and the kernels' KIND / DK template arguments count them
constexpr int DITHER_NONE = 0, DITHER_TRI = 1, DITHER_RECT = 2;

// C. Wellons' two-multiply integer hash.  The fast epilogues pass the multipliers from VGPRs they parked them in.
D2D_HD uint32_t lowbias32(uint32_t x, uint32_t c1 = 0x7feb352dU, uint32_t c2 = 0x846ca68bU) {
    x ^= x >> 16; x *= c1;
    x ^= x >> 15; x *= c2;
    x ^= x >> 16;
    return x;
}

// [own] counter-based dither generator, identical to orc_rng() in oracle/d2d_oracle.c: word = lowbias32(lo32(n) + k32 + hi32(n)*kstep).
// `lo` = lo32(n); the host folds hi32 of the call's first index into `key` (StreamJob::rng_key) and gives lo32 of that index as `lo0`:
// a call spans fewer than 2^32 outputs, so lo32(n) wraps at most once inside it, and where it has, `kstep` is due once more.
D2D_HD uint32_t dither_word(uint32_t lo, uint32_t key, uint32_t kstep, uint32_t lo0) {
    return lowbias32(lo + key + (lo < lo0 ? kstep : 0u));
}

// The generator's 64-bit key of one channel (oracle: orc_rng_key): the engine splits it into StreamJob::rng_key / rng_kstep per call, the
// host twins hash an absolute index on it directly (dither_word_at == orc_rng).
D2D_HD uint64_t dither_key64(uint64_t seed, uint32_t channel) {
    uint64_t z = (seed ^ ((uint64_t)channel * 0xD1B54A32D192ED03ull)) + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
D2D_HD uint32_t dither_word_at(uint64_t key64, uint64_t n) {
    const uint32_t kstep = (uint32_t)key64 | 1u;
    return lowbias32((uint32_t)n + (uint32_t)(key64 >> 32) + (uint32_t)(n >> 32) * kstep);
}

// The dither of the integer depths as an integer `term` of the hash word: triangular d = term * 2^-16 - 1 with term = lo16 + hi16 + 1,
// rectangular d = term * 2^-17 - 1/2 with term = 2 hi16 + 1 (both symmetric about zero, never zero-width at the ends)
template <int KIND>
D2D_HD uint32_t dither_term(uint32_t z) {
    if constexpr (KIND == DITHER_TRI) return (z & 0xFFFFu) + (z >> 16) + 1u;
    else if constexpr (KIND == DITHER_RECT) return 2u * (z >> 16) + 1u;
    else return 0u;
}
template <int KIND>
D2D_HD double dither_f64(uint32_t term) {      // exact: term < 2^18
    if constexpr (KIND == DITHER_TRI) return fma((double)term, 0x1p-16, -1.0);
    else if constexpr (KIND == DITHER_RECT) return fma((double)term, 0x1p-17, -0.5);
    else return 0.0;
}

// a7: round half away from zero, clip to [-lim, lim - 1]   (== q >= 0 ? floor(q + .5) : ceil(q - .5), clipped)
D2D_HD int32_t round_clip(double q, double lim) {
    return (int32_t)fmax(fmin(trunc(q + copysign(0.5, q)), lim - 1.0), -lim);
}

D2D_HD uint32_t f32_bits(float f) { return __builtin_bit_cast(uint32_t, f); }

// Airwindows "Dither Float" for 32-bit float output: x + (z - 0x7fffffff) * 5.5e-36 * 2^(expon + 62), frexpf((float)x) -> expon
// (0 for zero and subnormal floats), z the hash word.  The sample is the sum's (float).
D2D_HD double dither_float(double x, uint32_t z) {
    const uint32_t fb = f32_bits((float)x);
    const int e = (int)((fb >> 23) & 0xFFu);
    const int expon = e ? e - 126 : 0;
    const double t = ((double)z - 2147483647.0) * 5.5e-36;
    return x + ldexp(t, expon + 62);
}

// The all-integer requantiser of unit gain: x = v * 2^-F LSB with v = sum q s an integer and 0 < F <= 16, the dither an integer number
// of 2^-16 (rectangular: 2^-17) LSB -- the real numbers of round_clip(x + dither_f64<KIND>(dither_term<KIND>(z)), .), no f64 operation.
//   vh = floor(x), vl = its fraction; w = vl + d in 2^-16 (2^-17) LSB; neg = -1 where x + d < 0; rr = round half away from zero
template <int KIND>
D2D_HD int32_t requant_int_round(int32_t v, int F, uint32_t z) {
    const int32_t vh = v >> F;
    const uint32_t vl = (uint32_t)v & ((1u << F) - 1u);
    if constexpr (KIND == DITHER_RECT) {
        const int32_t w = (int32_t)(vl << (17 - F)) + (int32_t)(2u * (z >> 16) + 1u) - 65536;
        const int32_t neg = (vh + (w >> 17)) >> 31;
        return vh + ((w + 65536 + neg) >> 17);
    } else {
        int32_t w = (int32_t)(vl << (16 - F));
        if constexpr (KIND == DITHER_TRI) w += (int32_t)((z & 0xFFFFu) + (z >> 16)) - 65535;
        const int32_t neg = (vh + (w >> 16)) >> 31;
        return vh + ((w + 32768 + neg) >> 16);
    }
}
template <int KIND>
D2D_HD int32_t requant_int(int32_t v, int F, uint32_t z, int32_t qmin, int32_t qmax) {
    const int32_t rr = requant_int_round<KIND>(v, F, z);
    const int32_t lo = rr > qmin ? rr : qmin;
    return lo < qmax ? lo : qmax;
}

// The four balanced int8 limb sums of one output of the int8 matrix kernels hold 128 * sum q b; this is 2 * sum q b
// = (A0 >> 6) + 4*A1 + 2^10*A2 + 2^18*A3 modulo 2^32 (A0 is a multiple of 128; |2 sum q b - 2^S| < 2^31, so a wrap is harmless)
D2D_HD uint32_t recombine_limbs(int32_t A0, int32_t A1, int32_t A2, int32_t A3) {
    uint32_t u0 = (uint32_t)(A0 >> 6);
    u0 = ((uint32_t)A1 << 2) + u0;
    u0 = ((uint32_t)A2 << 10) + u0;
    u0 = ((uint32_t)A3 << 18) + u0;
    return u0;
}

}  // namespace d2d
