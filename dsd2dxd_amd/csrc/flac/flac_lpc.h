// flac_lpc.h -- the arithmetic of the rules at the head of flac_frame_enc.h that the host encoder and the GPU kernels must agree on
// bit for bit.  d2drice (every effort): Rice parameter, zigzag, pmax, the bits in front of a subframe's partitions.  d2dlpc (effort 12,
// rules 9 to 19): the window, the way from the autocorrelation to quantised coefficients, and the residual.  One copy, plain C++,
// compiled for the host (g++) and for the device (hipcc).
//
// The floating-point part, lpc_coefficients, is a short serial routine in IEEE f64: every operation is the single operation written,
// in the order written.  Both builds use -ffp-contract=off (no fused multiply-add); under clang the routine says so itself.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define D2D_LPC_HD __host__ __device__ __forceinline__
#else
#define D2D_LPC_HD inline
#endif
#if defined(__clang__)
#define D2D_LPC_UNROLL _Pragma("unroll")       // the device keeps the routine's arrays in registers
#else
#define D2D_LPC_UNROLL
#endif

namespace d2drice {

constexpr uint32_t SUBFRAME_BITS = 8, METHOD_BITS = 6, PARAM_BITS = 5;      // 0 tttttt 0;  01 pppp;  a partition's kkkkk

// the smallest k with 2^k >= floor(sum / count), at most 30 (rule 4); sum is a partition's sum |r|
D2D_LPC_HD uint32_t rice_k(uint64_t sum, uint32_t count) {
    const uint64_t mean = sum / (count ? count : 1);
    uint32_t k = 0;
    while (k < 30 && (1ull << k) < mean) ++k;
    return k;
}
// u = 2 r for r >= 0, -2 r - 1 below: what the code writes; |r| = (u + 1) >> 1
D2D_LPC_HD uint32_t zigzag(int32_t r) { return r >= 0 ? (uint32_t)r << 1 : ((uint32_t)(-(int64_t)r) << 1) - 1; }
// the largest p <= 6 with n % 2^p == 0 and (n >> p) >= 16 (rule 6)
D2D_LPC_HD uint32_t search_pmax(uint32_t n) {
    uint32_t p = 0;
    while (p < 6 && n % (2u << p) == 0 && (n >> (p + 1)) >= 16) ++p;
    return p;
}
// the bits in front of the partitions of a subframe of b-bit samples: fixed order o (rule 4); LPC order P (rule 15: 1101 sssss, P q's)
D2D_LPC_HD uint32_t fixed_header_bits(uint32_t o, uint32_t b) { return SUBFRAME_BITS + o * b + METHOD_BITS; }
D2D_LPC_HD uint32_t lpc_coef_bits(uint32_t P) { return 4 + 5 + 14 * P; }
D2D_LPC_HD uint32_t lpc_header_bits(uint32_t P, uint32_t b) { return fixed_header_bits(P, b) + lpc_coef_bits(P); }

}  // namespace d2drice

namespace d2dlpc {

constexpr int MAX_ORDER = 12;                  // the highest order searched; the candidates are 4, 8 and 12
constexpr int CANDIDATES = 3;
constexpr uint32_t MIN_FRAME = 64;             // shorter frames have no LPC candidates
constexpr int PRECISION = 14;                  // bits of a quantised coefficient

struct LpcCoefs {
    int32_t q[CANDIDATES][MAX_ORDER];          // q[c][j - 1] multiplies x(i - j); candidate c has order 4 (c + 1)
    int32_t shift[CANDIDATES];
    uint32_t valid;                            // bit c: candidate c exists
};

// s of rule 11: the bit length of the window's maximum, floor((n + 1) / 2) floor((n + 2) / 2)
D2D_LPC_HD uint32_t lpc_window_shift(uint32_t n) {
    const uint64_t top = (uint64_t)((n + 1) / 2) * ((n + 2) / 2);
    uint32_t s = 0;
    while (top >> s) ++s;
    return s;
}
// y(i) = (x(i) w(i)) >> s, w(i) = (i + 1)(n - i), i < n
D2D_LPC_HD int32_t lpc_window(int32_t x, uint32_t i, uint32_t n, uint32_t s) {
    return (int32_t)(((int64_t)x * (int64_t)((uint64_t)(i + 1) * (n - i))) >> s);
}

// x(i) - ((sum over j = 1 .. P of q[j - 1] x(i - j)) >> shift); before[j - 1] = x(i - j)
template <int P>
D2D_LPC_HD int32_t lpc_residual(int32_t x, const int32_t* before, const int32_t* q, int32_t shift) {
    int64_t sum = 0;
D2D_LPC_UNROLL
    for (int j = 0; j < P; ++j) sum += (int64_t)q[j] * before[j];
    return (int32_t)(x - (sum >> shift));
}

// a[1 .. m] -> candidate `slot` (rule 13): shift, error-feedback quantisation, the drop at sum |q| > 62 * 2^shift
template <int M>
D2D_LPC_HD void lpc_quantise(const double* a, LpcCoefs& c, int slot) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    double cmax = 0.0;
    bool in_range = true;
D2D_LPC_UNROLL
    for (int j = 1; j <= M; ++j) {
        const double v = fabs(a[j]);
        if (!(v < 8192.0)) in_range = false;   // 2^13: the shift would be negative (and anything not finite ends here)
        if (v > cmax) cmax = v;
    }
    if (!in_range || cmax == 0.0) return;
    int e = 0;
    (void)frexp(cmax, &e);                      // cmax = f 2^e, 1/2 <= f < 1: the smallest e with cmax < 2^e
    const int shift = 13 - e > 15 ? 15 : 13 - e;
    const double scale = (double)(1 << shift);
    double t = 0.0;
    int64_t total = 0;
D2D_LPC_UNROLL
    for (int j = 1; j <= M; ++j) {
        t = t + a[j] * scale;
        double v = floor(t + 0.5);
        v = v < -8192.0 ? -8192.0 : v > 8191.0 ? 8191.0 : v;
        t = t - v;
        const int32_t q = (int32_t)v;
        c.q[slot][j - 1] = q;
        total += q < 0 ? -q : q;
    }
    if (total > ((int64_t)62 << shift)) return;
    c.shift[slot] = shift;
    c.valid |= 1u << slot;
}

// R(0 .. 12) -> the candidates (rule 13): the Levinson-Durbin recursion, stopped for good the first time the error is not positive
D2D_LPC_HD void lpc_coefficients(const int64_t* R, LpcCoefs& c) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    c.valid = 0;
    if (R[0] == 0) return;
    double r[MAX_ORDER + 1], a[MAX_ORDER + 1];
D2D_LPC_UNROLL
    for (int l = 0; l <= MAX_ORDER; ++l) { r[l] = (double)R[l]; a[l] = 0.0; }
    double err = r[0];
D2D_LPC_UNROLL
    for (int m = 1; m <= MAX_ORDER; ++m) {
        double acc = r[m];
D2D_LPC_UNROLL
        for (int j = 1; j < m; ++j) acc = acc - a[j] * r[m - j];
        const double k = acc / err;
D2D_LPC_UNROLL
        for (int j = 1; 2 * j <= m; ++j) {          // a'[j] = a[j] - k a[m - j], a pair at a time: every a' from the old a
            const double lo = a[j], hi = a[m - j];
            a[j] = lo - k * hi;
            a[m - j] = hi - k * lo;
        }
        a[m] = k;
        err = err * (1.0 - k * k);
        if (!(err > 0.0)) return;
        if (m == 4) lpc_quantise<4>(a, c, 0);
        if (m == 8) lpc_quantise<8>(a, c, 1);
        if (m == 12) lpc_quantise<12>(a, c, 2);
    }
}

}  // namespace d2dlpc
