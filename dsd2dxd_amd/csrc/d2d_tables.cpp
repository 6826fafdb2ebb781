// d2d_tables.cpp -- the host-side construction of every device table from the frozen designs in filters/filter_tables.inc.  No HIP call.
#include "d2d_tables.h"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>

namespace d2d {

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
// 2 q has to fit five digits: |2q| <= 16 * (32^5 - 1) / 31
static bool fits_five_digits(int64_t q2) { return !(q2 > 16236247 || q2 < -17318416); }

// One lane of an fp6 tap fragment [64 lanes x 16 bytes | 64 lanes x 8 bytes] from its 32 digits (0: no tap there).  Element j is a 6-bit e2m3
// code at bits [6j, 6j+6) of the lane's 192; it meets B register j >> 3, which arrives as 0.5 (even register) or 1.0 (odd): d/4 or d/8.
static void pack_lane(int8_t* frag, int l, const int d[32]) {
    uint32_t regs[6] = {0, 0, 0, 0, 0, 0};
    for (int j = 0; j < 32; ++j) {
        const uint32_t code = e2m3_code(((j >> 3) & 1) ? d[j] * 0.125 : d[j] * 0.25);
        for (int b = 0; b < 6; ++b) if ((code >> b) & 1) regs[(6 * j + b) >> 5] |= 1u << ((6 * j + b) & 31);
    }
    memcpy(frag + (size_t)l * 16, regs, 16);
    memcpy(frag + 1024 + (size_t)l * 8, regs + 4, 8);
}

static uint64_t sum_abs(const int32_t* q, int n) {
    uint64_t sa = 0;
    for (int j = 0; j < n; ++j) sa += (uint64_t)(q[j] < 0 ? -(int64_t)q[j] : (int64_t)q[j]);
    return sa;
}
uint64_t sum_abs_q(const d2d_filter_def& f) { return 2 * sum_abs(f.half, f.ntaps / 2); }    // (the stored half, mirrored)
uint64_t max_phase_sum_abs(const d2d_poly_def& p) {
    uint64_t sa = 0;
    for (int ph = 0; ph < p.Lp; ++ph) sa = std::max(sa, sum_abs(p.q + (size_t)ph * p.NP, p.NP));
    return sa;
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
    for (int k = 0; k < f.ntaps; ++k) if (!fits_five_digits(2 * (int64_t)tap_q(f, k))) return false;
    return f.S >= 20 && f.S <= 30 && lo < (1 << 24) && hi < (1 << 24);
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

// The polyphase kernel recombines v = lo + 2^15 hi with lo = S0 + 32 S1 + 2^10 S2 and hi = S3 + 32 S4 in f32: exact while every value that can
// occur stays below 2^24; a digit sum over any subset of a window's bits is bounded by the sum of the digits' magnitudes (per phase).
bool px_exact(const d2d_poly_def& p) {
    if (p.S < 20 || p.S > 30) return false;
    for (int ph = 0; ph < p.Lp; ++ph) {
        int64_t sa[5] = {0, 0, 0, 0, 0}, sq = 0;
        for (int j = 0; j < p.NP; ++j) {
            const int64_t q = p.q[(size_t)ph * p.NP + j], q2 = 2 * q;
            if (!fits_five_digits(q2)) return false;
            sq += q;
            for (int l = 0; l < 5; ++l) { const int d = digit32(q2, l); sa[l] += d < 0 ? -d : d; }
        }
        if (sq != ((int64_t)1 << p.S)) return false;                       // the accumulators' start value assumes unity DC gain per phase
        const int64_t lo = sa[0] + 32 * sa[1] + 1024 * sa[2], hi = sa[3] + 32 * (sa[4] + ((int64_t)1 << (p.S - 20)));
        if (lo >= (1 << 24) || hi >= (1 << 24)) return false;
    }
    return true;
}

d2d_filter_def residual_def(const d2d_filter_def& f, std::vector<int32_t>& storage) {
    storage.resize((size_t)f.ntaps / 2);
    for (int k = 0; k < f.ntaps / 2; ++k) storage[(size_t)k] = (int32_t)((int64_t)f.half32[k] - (int64_t)f.half[k] * 256);
    d2d_filter_def lo = f; lo.half = storage.data(); lo.half32 = nullptr;
    return lo;
}

// Nibble tables [ntab][16] of f64.  Table pad+2w serves the HIGH nibble of window byte w, table
// pad+2w+1 its LOW nibble, whatever the stream's bit order: for MSB-first streams the high nibble
// holds the four EARLIER samples (bit 7 first), for LSB-first streams the LATER four (bit 4 first).
std::vector<double> build_lut_tables(const d2d_filter_def& f, int MB, bool msb_first) {
    const int Wb = f.ntaps / 8;
    const LutLayout g = lut_layout(MB, Wb);
    std::vector<double> t((size_t)g.ntab * 16, 0.0);
    const double scale = 1.0 / (double)(1ull << f.S);   // exact power of two
    for (int w = 0; w < Wb; ++w)
        for (int nib = 0; nib < 2; ++nib)              // 0 = high nibble of the byte, 1 = low nibble
            for (int x = 0; x < 16; ++x) {
                int64_t acc = 0;
                for (int i = 0; i < 4; ++i) {
                    // bit i of the nibble value x  ->  time position inside the byte
                    int tpos = msb_first ? (nib == 0 ? 3 - i : 7 - i) : (nib == 0 ? 4 + i : i);
                    int64_t q = tap_q(f, 8 * w + tpos);
                    acc += ((x >> i) & 1) ? q : -q;
                }
                t[(size_t)(g.pad + 2 * w + nib) * 16 + x] = (double)acc * scale;
            }
    return t;
}

// Tap fragments [4 byte shifts][ksteps + 6][64 lanes][16 bytes].  Lane l supplies matrix row (l & 31) = 4*phase + limb
// for the K slots (l >> 5)*16 + j; slot (ks, h, j) reads bit `wb` of the row window (see the
// kernel's A00/A01), which sits at bit position p = wb & 7 of its stream byte and therefore arrives
// as 2^p (p = 7: -128): the table holds q * 2^(7-p), negated for p = 7.
std::vector<int8_t> build_mfma_tables(const d2d_filter_def& f, const MfmaLayout& g, bool msb_first) {
    const int U = g.ksteps / 2;
    const size_t per = (size_t)(g.ksteps + 6) * 64 * 16;           // +6 zero steps: the kernel's read-ahead
    std::vector<int8_t> t(4 * per, 0);
    for (int sh = 0; sh < 4; ++sh)                                  // window starts `sh` bytes into its first dword
        for (int ks = 0; ks < g.ksteps; ++ks)
            for (int l = 0; l < 64; ++l) {
                const int row = l & 31, h = l >> 5, limb = row & 3;
                // D row i lands in lane half (i >> 2) & 1, register group i >> 3: give that slot output
                // phase 4*half + group, so lane (r, half) owns the four CONSECUTIVE outputs 8r + 4*half + k
                const int ph = 4 * ((row >> 2) & 1) + (row >> 3);
                for (int j = 0; j < 16; ++j) {
                    const int p = 4 * (ks & 1) + (j >> 2);                        // register v = j>>2 of step ks
                    const int wb = 32 * (h * U + (ks >> 1)) + 8 * (j & 3) + p;     // bit of the LDS row words
                    const int tau = (msb_first ? (wb & ~7) + 7 - (wb & 7) : wb) - 8 * sh;   // its time index in the window
                    const int tap = tau - ph * g.M;
                    int8_t v = 0;
                    if (tau >= 0 && tap >= 0 && tap < f.ntaps) {
                        int64_t q = tap_q(f, tap);
                        q = p == 7 ? -q : q * (int64_t)(1 << (7 - p));
                        v = limb256(q, limb);
                    }
                    t[sh * per + ((size_t)ks * 64 + l) * 16 + j] = v;
                }
            }
    return t;
}

// Tap fragments [4 byte shifts][2*NPG][64 lanes][16 bytes].  Fragment 2*pp + n serves pair step pp of a
// group's window, bit positions 4n .. 4n+3 of every byte.  Lane l supplies matrix row (l & 31) =
// 4*slot + limb for the K slots of lane half hh = l >> 5, i.e. the staged dword 2*pp + hh of the window;
// slot j of the lane = byte (j & 3), plane (j >> 2) -> bit position p = 4n + (j >> 2) of that byte,
// which arrives as 2^p (p = 7: -128): the table holds q * 2^(7-p), negated for p = 7.
std::vector<int8_t> build_mfma2_tables(const d2d_filter_def& f, bool msb_first, bool unmask0_wanted) {
    const int NPG = mfma2_pairs(f.M, f.ntaps);
    const bool unmask0 = unmask0_wanted && m2_unmask0(NPG);
    const size_t per = (size_t)(2 * NPG) * 64 * 16;
    std::vector<int8_t> t(4 * per, 0);
    for (int sh = 0; sh < 4; ++sh)                                  // window starts `sh` bytes into its first dword
        for (int fr = 0; fr < 2 * NPG; ++fr)
            for (int l = 0; l < 64; ++l) {
                const int pp = fr >> 1, n = fr & 1;
                const int row = l & 31, hh = l >> 5, limb = row & 3;
                // D row i lands in lane half (i >> 2) & 1, register group i >> 3: give that slot output
                // phase 4*half + group, so lane (r, half) owns the four CONSECUTIVE outputs 4*half + k of a group
                const int ph = 4 * ((row >> 2) & 1) + (row >> 3);
                for (int j = 0; j < 16; ++j) {
                    const int p = 4 * n + (j >> 2);
                    auto entry = [&](int pp_) -> int64_t {                                   // q * 2^(7-p) (p = 7: -q) of bit position pp_ of this byte
                        const int wb_ = 32 * (2 * pp + hh) + 8 * (j & 3) + pp_;                    // bit of the staged window
                        const int tau_ = (msb_first ? (wb_ & ~7) + 7 - (wb_ & 7) : wb_) - 8 * sh;  // its time index in the window
                        const int tap_ = tau_ - ph * f.M;
                        if (tau_ < 0 || tap_ < 0 || tap_ >= f.ntaps) return 0;
                        const int64_t q = tap_q(f, tap_);
                        return pp_ == 7 ? -q : q * (int64_t)(1 << (7 - pp_));
                    };
                    int64_t T = entry(p);
                    if (unmask0 && p != 0) T -= entry(0);                                 // plane 0 arrives unmasked (see the kernel)
                    t[sh * per + ((size_t)fr * 64 + l) * 16 + j] = limb256(T, limb);
                }
            }
    return t;
}

// Tap fragments: [4 byte shifts][NF fragments][64 lanes x 16 bytes | 64 lanes x 8 bytes].  Fragment f multiplies the stream dwords
// 2f (lane half 0) and 2f + 1 (half 1) of a column's window.  A lane l = matrix row l & 31, K half l >> 5; its element j (pack_lane)
// meets B register p = j >> 3, nibble n = j & 7 = bit 4n + p of the dword.  D row i lands in lane half (i >> 2) & 1, register
// 4 (i >> 3) + (i & 3) = 5 q + digit: phase 3 half + q (wide: register 7 q + digit, phase 2 half + q).
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
                int d[32] = {};
                if (rho < PHH * ND) {
                    const int ph = PHH * half + rho / ND, dg = rho % ND;
                    for (int j = 0; j < 32; ++j) {
                        const int p = j >> 3, n = j & 7;
                        const int wb = 32 * (2 * fr + kh) + 4 * n + p;                             // bit of the staged window
                        const int tau = (msb_first ? (wb & ~7) + 7 - (wb & 7) : wb) - 8 * sh;     // its time index in the window
                        const int tap = tau - ph * M;
                        if (tau < 0 || tap < 0 || tap >= N) continue;
                        d[j] = digit32(wide ? 2 * tap_q32(f, tap) : 2 * (int64_t)tap_q(f, tap), dg);
                    }
                }
                pack_lane(&t[sh * per + (size_t)fr * MX_FRAG_BYTES], l, d);
            }
    return t;
}

// Tap fragments [slot (step u, group g) in issue order][64 lanes x 16 bytes | 64 lanes x 8 bytes].  A lane l = matrix row l & 31, K half
// l >> 5; its element e (pack_lane) meets B register e >> 3, nibble e & 7 = bit 4 (e & 7) + (e >> 3) of the lane half's dword = bit
// x = 64 u + 32 (l >> 5) + that of the column's window.  D row i lands in lane half (i >> 2) & 1, register 4 (i >> 3) + (i & 3) = 5 i' + digit:
// output 3 half + i' of the group.  Output o of the column (o = 5 g + 3 half + i') meets window bit x with tap j = q_o + NP - 1 - x of phase
// (o Mp) mod Lp.
std::vector<int8_t> build_px_tables(const d2d_poly_def& p) {
    const int G = px_groups(p), LP = p.Lp, MP = p.Mp, NP = p.NP;
    const int TP = px_tp(LP, MP, NP, G), NSLOT = px_nslot(LP, MP, NP, G);
    std::vector<int8_t> t((size_t)NSLOT * PX_FRAG_BYTES, 0);
    for (int u = 0; u < TP; ++u)
        for (int g = 0; g < G; ++g) {
            if (!px_active(LP, MP, NP, u, g)) continue;
            int8_t* fbp = &t[(size_t)px_slot(LP, MP, NP, G, u, g) * PX_FRAG_BYTES];
            for (int l = 0; l < 64; ++l) {
                const int row = l & 31, kh = l >> 5;
                const int half = (row >> 2) & 1, rr = 4 * (row >> 3) + (row & 3);
                int d[32] = {};
                const int ii = rr / 5, dg = rr % 5;
                const int og = 3 * half + ii < 5 ? 3 * half + ii : 4;         // (half 1's third slot repeats output 4: a real sample for the pipelined epilogue's extremes, stored nowhere)
                if (rr < 15) {
                    const int o = 5 * g + og;
                    const int qo = px_q(LP, MP, o), ph = (int)(((long long)o * MP) % LP);
                    for (int e = 0; e < 32; ++e) {
                        const int x = 64 * u + 32 * kh + 4 * (e & 7) + (e >> 3);
                        const int j = qo + NP - 1 - x;
                        if (j < 0 || j >= NP) continue;
                        d[e] = digit32(2 * (int64_t)p.q[(size_t)ph * NP + j], dg);
                    }
                }
                pack_lane(fbp, l, d);
            }
        }
    return t;
}

uint32_t resamp2_nstep(const d2d_resamp_def& r) {
    int need = 0;
    for (int rho = 0; rho < r.L / 4; ++rho) {
        const int b0 = (r.Mdn * 4 * rho) / r.L, b3 = (r.Mdn * (4 * rho + 3)) / r.L;
        need = std::max(need, b3 + r.P - (b0 & ~15));
    }
    return (uint32_t)((need + 63) / 64);
}

// [L/4 blocks][NSTEP][64 lanes][16 bytes], then the blocks' row offsets (uint32, padded to 16 bytes).  A lane l = matrix row l & 15
// = (phase p = row / 4, digit a = row % 4), K group l / 16; its byte j is K slot kappa = 64 s + 16 (l / 16) + j = the row's sample
// rowoff + kappa = X[147 c - (P-1) + rowoff + kappa], which tap k = b_r + (P-1) - rowoff - kappa of residue r = 4 rho + p multiplies.
std::vector<int8_t> build_resamp2_table(const d2d_resamp_def& r) {
    const int NB = r.L / 4, NSTEP = (int)resamp2_nstep(r);
    std::vector<int8_t> t((size_t)NB * NSTEP * 1024 + (((size_t)NB * 4 + 15) & ~(size_t)15), 0);
    uint32_t* ro = reinterpret_cast<uint32_t*>(t.data() + (size_t)NB * NSTEP * 1024);
    for (int rho = 0; rho < NB; ++rho) {
        const int rowoff = ((r.Mdn * 4 * rho) / r.L) & ~15;
        ro[rho] = (uint32_t)rowoff;
        for (int s = 0; s < NSTEP; ++s)
            for (int l = 0; l < 64; ++l) {
                const int row = l & 15, p = row >> 2, a_ = row & 3, kgp = l >> 4;
                const int res = 4 * rho + p, b = (r.Mdn * res) / r.L, phase = (r.Mdn * res) % r.L;
                for (int j = 0; j < 16; ++j) {
                    const int kappa = 64 * s + 16 * kgp + j;
                    const int k = b + (r.P - 1) - rowoff - kappa;
                    if (k < 0 || k >= r.P) continue;
                    t[((size_t)(rho * NSTEP + s) * 64 + l) * 16 + j] = limb256((int64_t)r.q[(size_t)phase * r.P + k], a_);
                }
            }
    }
    return t;
}

std::vector<int8_t> build_fir_table(const d2d_filter_def& f, int pipe, bool two_group, const MfmaLayout& layout, bool msb_first, bool wide) {
    return pipe == PIPE_FP6 ? build_mx_tables(f, msb_first, wide)
         : two_group ? build_mfma2_tables(f, msb_first, !pipe) : build_mfma_tables(f, layout, msb_first);
}

}  // namespace d2d
