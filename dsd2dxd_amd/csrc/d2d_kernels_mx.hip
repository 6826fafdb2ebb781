// d2d_kernels_mx.hip -- the FIR decimator on the fp6 x fp4 matrix-core instruction (gfx950), exact, software-pipelined.
//
// Same arithmetic contract, staging, pipelining and epilogue as d2d_kernels_mfma3.hip (stereo at 0 dB: 24-bit, 16-bit, float frames,
// and the exact integers for the stage-A / noise-shaper scratch); what changes is the instruction that carries the dot product and,
// with it, the geometry.  v_mfma_i32_32x32x32_i8 spends 32 cycles on 32 stream bits per column; v_mfma_scale_f32_32x32x64_f8f6f4
// with an fp6 (e2m3) A operand and an fp4 (e2m1) B operand spends the same 32 cycles on 64 (tools/ubench/mfma_shapes.hip), and one
// v_and turns a stream dword into EIGHT operand slots instead of four:
//
//   * B operand = the bit stream.  A nibble that holds one stream bit is an e2m1 number: 0b0001 = 0.5, 0b0010 = 1.0.  A stream dword W
//     becomes the lane's four operand registers W & 0x11111111, W & 0x22222222, (W >> 2) & 0x11111111, (W >> 2) & 0x22222222 (five
//     vector instructions for 32 bits; the int8 form needs eight): K slot 8p + n of the lane is bit 4n + p of its dword.
//   * A operand = the taps.  2q (q the 24-bit tap) is written in five balanced base-32 digits d in [-16, 15]; the slot that meets a
//     0.5-valued bit holds d/4, the slot that meets a 1.0-valued bit d/8 -- both exact in e2m3 (multiples of 1/8 up to 2, of 1/4 up to
//     4) -- and the B scale of the instruction is 2^3, so every product is the integer d * bit and the f32 accumulators hold the exact
//     digit sums (|sum| <= 16 * 752 << 2^24).  Matrix row = (phase, digit): 6 phases x 5 digits = 30 of the 32 rows; a lane half owns
//     the three phases 3h .. 3h+2 of every group with all five digits of a sample in its own registers.
//   * v = sum q s = S0 + 32 S1 + 2^10 S2 + 2^15 (S3 + 32 S4), accumulators started from -2^S in the digit-4 rows: two f32 fma
//     (|.| < 2^24: exact), one more for the high part, two conversions, one shift-add.
//   * One matrix column serves 6 G consecutive outputs (G groups of six phases); group g reads the tap fragments of group 0
//     6 M / 64 steps later, a step being 64 stream bits (lane half h takes dword 2u + h).  M = 32, E filter: 12 fragments, 15 steps and
//     24 MFMAs per 384 outputs = 32 per 512 (the int8 form: 52), 100 operand-expansion instructions per 512 outputs (136).
//   * The stereo frame flavours at M = 32 hold their (at most twelve) fragments in registers for the life of a wave instead of reading
//     them from LDS in every chain; the registers are those of the draining accumulator set, emptied in one burst at the start of a
//     region (d2d_mx.h: mx_resident; d2d_mx_kernel.h: RES, burst).
//
// Frames leave through a per-wave LDS slice (a lane owns runs of three samples, not of four): samples in as dwords, out as groups of
// four frames, packed and stored as in the int8 kernel.
//
// Replaces: the per-block translate loop inside Rdsd2Pcm::do_conversion
// (/root/reference/src/main.rs:345,429); the crate that holds it is absent from the reference.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "d2d_mx_kernel.h"

namespace d2d {

// ---- host side -------------------------------------------------------------------------------
// This object is unit 0 of D2D_MX_UNIT_LIST (the E_M32 shape's integer kernels) and holds the table builder and the dispatcher.
#define X(unit, mb, nt, fl, npr) +1
static_assert(D2D_MX_UNITS == 0 D2D_MX_UNIT_LIST(X), "the Makefile's MX_UNITS is not the length of D2D_MX_UNIT_LIST (d2d_mx.h)");
#undef X
#define X(unit, mb, nt, fl, npr) extern template hipError_t launch_mx_unit<unit>(Mfma2Args& m, uint32_t max_nout, uint32_t nrows, hipStream_t s);
D2D_MX_UNIT_LIST(X)
#undef X
template hipError_t launch_mx_unit<0>(Mfma2Args& m, uint32_t max_nout, uint32_t nrows, hipStream_t s);

struct MxRow { int MB, NT; MxFlavour fl; int npr; hipError_t (*fn)(Mfma2Args&, uint32_t, uint32_t, hipStream_t); };
static const std::vector<MxRow>& mx_rows() {
    static const std::vector<MxRow> rows = [] {
        std::vector<MxRow> v;
#define X(unit, mb, nt, fl, npr) if constexpr (mx_unit_kept(mb, nt)) v.push_back({mb, nt, fl, npr, &launch_mx_unit<unit>});
        D2D_MX_UNIT_LIST(X)
#undef X
        return v;
    }();
    return rows;
}
static const MxRow* mx_find(int MB, int NT, MxFlavour fl, int npr) {
    for (const MxRow& r : mx_rows()) if (r.MB == MB && r.NT == NT && r.fl == fl && r.npr == npr) return &r;
    return nullptr;
}
bool mx_supported(int MB, int NT) { return mx_find(MB, NT, MX_INT, 1) != nullptr; }
bool mx_pairs_supported(int MB, int NT, int npairs) { return npairs > 1 && mx_find(MB, NT, MX_INT, npairs) != nullptr; }
bool mx_wide_supported(int MB, int NT) { return mx_find(MB, NT, MX_WIDE, 1) != nullptr; }
bool mx_gain_supported(int MB, int NT) { return mx_find(MB, NT, MX_GAIN, 1) != nullptr; }

// e2m3 code of x (a multiple of 1/8 up to 2, of 1/4 up to 4, of 1/2 up to 7.5)
static uint32_t e2m3_code(double x) {
    const uint32_t s = x < 0 ? 32u : 0u;
    const double ax = fabs(x);
    for (uint32_t c = 0; c < 32; ++c) {
        const uint32_t e = c >> 3, mm = c & 7;
        const double v = e ? (1.0 + mm / 8.0) * (double)(1 << (e - 1)) : mm * 0.125;
        if (v == ax) return ax == 0 ? 0u : (s | c);
    }
    fprintf(stderr, "d2d: %g is not an e2m3 number\n", x);
    abort();
}
// balanced base-32 digit l of v: v = sum d_l 32^l, every d in [-16, 15]
static int digit32(int64_t v, int l) {
    int dd = 0;
    for (int i = 0; i <= l; ++i) {
        dd = (int)(((v + 16) & 31) - 16);
        v = (v - dd) / 32;
    }
    return dd;
}

// The recombination v = lo + 2^15 hi with lo = S0 + 32 S1 + 2^10 S2 and hi = S3 + 32 S4 is done in f32: exact while every value that can
// occur stays below 2^24.  A digit sum over ANY subset of the window's bits is bounded by the sum of the digits' magnitudes.
bool mx_exact(const d2d_filter_def& f) {
    int64_t sa[5] = {0, 0, 0, 0, 0};
    for (int k = 0; k < f.ntaps; ++k)
        for (int l = 0; l < 5; ++l) { const int d = digit32(2 * (int64_t)tap_q(f, k), l); sa[l] += d < 0 ? -d : d; }
    // the kernel's two f32 parts: digits 0-2 | 3-4 (M = 128: 0-1 | 2-4), the -2^S start value in digit 4
    const bool s23 = f.M == 128;
    const int64_t lo = s23 ? sa[0] + 32 * sa[1] : sa[0] + 32 * sa[1] + 1024 * sa[2];
    const int64_t hi = s23 ? sa[2] + 32 * sa[3] + 1024 * (sa[4] + ((int64_t)1 << (f.S - 20))) : sa[3] + 32 * (sa[4] + ((int64_t)1 << (f.S - 20)));
    // 2 q has to fit five digits: |2q| <= 16 * (32^5 - 1) / 31
    for (int k = 0; k < f.ntaps; ++k) { const int64_t q2 = 2 * (int64_t)tap_q(f, k); if (q2 > 16236247 || q2 < -17318416) return false; }
    return f.S >= 20 && f.S <= 30 && lo < (1 << 24) && hi < (1 << 24);
}

// Tap fragments: [4 byte shifts][NF fragments][64 lanes x 16 bytes | 64 lanes x 8 bytes].  Fragment f multiplies the stream dwords
// 2f (lane half 0) and 2f + 1 (half 1) of a column's window.  A lane l = matrix row l & 31, K half l >> 5; its element j (a 6-bit
// e2m3 code at bits [6j, 6j+6) of the lane's 192) meets B register p = j >> 3, nibble n = j & 7 = bit 4n + p of the dword, which
// arrives as 0.5 (p even) or 1.0 (p odd).  D row i lands in lane half (i >> 2) & 1, register 4 (i >> 3) + (i & 3) = 5 q + digit:
// phase 3 half + q (wide: register 7 q + digit, phase 2 half + q).
// full 32-bit tap j (0..N-1) of the 2^-(S+8) grid (filters/filter_tables.inc: half32), stored like the 24-bit halves
static inline int64_t tap_q32(const d2d_filter_def& f, int j) {
    const int h = f.ntaps / 2;
    return j >= h ? f.half32[j - h] : f.half32[h - 1 - j];
}
// the one-pass form of the 32-bit grid: 2 q32 in seven balanced base-32 digits, v = lo + 2^15 mid + 2^25 hi with lo = S0 + 32 S1 + 2^10 S2,
// mid = S3 + 32 S4, hi = S5 + 32 S6, each formed in f32 (accumulators from zero; the -2^(S+8) is subtracted in 64 bits)
bool mx_wide_exact(const d2d_filter_def& f) {
    if (!f.half32) return false;
    int64_t sa[7] = {0, 0, 0, 0, 0, 0, 0};
    for (int k = 0; k < f.ntaps; ++k) {
        const int64_t q2 = 2 * tap_q32(f, k);
        int64_t back = 0, w = 1;
        for (int l = 0; l < 7; ++l) { const int d = digit32(q2, l); sa[l] += d < 0 ? -d : d; back += d * w; w *= 32; }
        if (back != q2) return false;                                  // 2 q32 does not fit seven digits
    }
    const int64_t lo = sa[0] + 32 * sa[1] + 1024 * sa[2], mid = sa[3] + 32 * sa[4], hi = sa[5] + 32 * sa[6];
    return f.S + 8 >= 28 && f.S + 8 <= 40 && lo < (1 << 24) && mid < (1 << 24) && hi < (1 << 24);
}

std::vector<int8_t> build_mx_tables(const d2d_filter_def& f, bool msb_first, bool wide) {
    const int M = f.M, N = f.ntaps, MB = M / 8;
    const int PH = wide ? 4 : 6, PHH = PH / 2, ND = wide ? 7 : 5;
    const int NF = mx_nf(MB, N, PH);
    const size_t per = (size_t)NF * MX_FRAG_BYTES;
    std::vector<int8_t> t(4 * per, 0);
    for (int sh = 0; sh < 4; ++sh)
        for (int fr = 0; fr < NF; ++fr)
            for (int l = 0; l < 64; ++l) {
                const int row = l & 31, kh = l >> 5;
                const int half = (row >> 2) & 1, rho = 4 * (row >> 3) + (row & 3);
                uint32_t regs[6] = {0, 0, 0, 0, 0, 0};
                if (rho < PHH * ND) {
                    const int ph = PHH * half + rho / ND, dg = rho % ND;
                    for (int j = 0; j < 32; ++j) {
                        const int p = j >> 3, n = j & 7;
                        const int wb = 32 * (2 * fr + kh) + 4 * n + p;                             // bit of the staged window
                        const int tau = (msb_first ? (wb & ~7) + 7 - (wb & 7) : wb) - 8 * sh;     // its time index in the window
                        const int tap = tau - ph * M;
                        if (tau < 0 || tap < 0 || tap >= N) continue;
                        const int d = digit32(wide ? 2 * tap_q32(f, tap) : 2 * (int64_t)tap_q(f, tap), dg);
                        const uint32_t code = e2m3_code((p & 1) ? d * 0.125 : d * 0.25);
                        for (int b = 0; b < 6; ++b) if ((code >> b) & 1) regs[(6 * j + b) >> 5] |= 1u << ((6 * j + b) & 31);
                    }
                }
                int8_t* fb = &t[sh * per + (size_t)fr * MX_FRAG_BYTES];
                memcpy(fb + (size_t)l * 16, regs, 16);
                memcpy(fb + 1024 + (size_t)l * 8, regs + 4, 8);
            }
    return t;
}

hipError_t launch_fir_mx(Mfma2Args& m, int MB, int NT, uint32_t max_nout, uint32_t nrows, hipStream_t s) {
    const MxRow* r = m.f.taps32 ? mx_find(MB, NT, MX_WIDE, 1)
                   : m.npairs > 1 ? mx_find(MB, NT, MX_INT, (int)m.npairs)
                   : m.gainq && !m.f.to_scratch ? mx_find(MB, NT, MX_GAIN, 1)
                   : mx_find(MB, NT, MX_INT, 1);
    return r ? r->fn(m, max_nout, nrows, s) : hipErrorInvalidValue;
}
int mx_groups(int MB) { return mx_g(MB); }
#if D2D_MX_STAMPS
void mx_debug_stamps(unsigned long long out[8]) {
    (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(d2d_mx_stamps), sizeof(unsigned long long) * 8);
    unsigned long long z[8] = {~0ull, 0, 0, 0, 0, 0, 0, 0};
    (void)hipMemcpyToSymbol(HIP_SYMBOL(d2d_mx_stamps), z, sizeof(z));
}
#else
void mx_debug_stamps(unsigned long long out[8]) { for (int i = 0; i < 8; ++i) out[i] = 0; }
#endif

}  // namespace d2d
