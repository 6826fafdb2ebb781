// d2d_tables.h -- every operand table the kernels read, built on the host (d2d_tables.cpp), the predicates and sums that gate kernel choice, and
// the geometry that builders and launchers share.  The unit calls no HIP function: tools/table_probe.cpp builds from it with g++ alone and
// prints a digest of every table, which tests/golden/table_digests.json pins (tests/test_tables_cpu.py).
#pragma once
#include "d2d_filters.h"
#include "d2d_internal.h"
#include "d2d_mx.h"
#include "d2d_px.h"

namespace d2d {

// full tap j (0..N-1) as the integer q_j (tap = q_j * 2^-S); 2nd half stored centre-outward
inline int32_t tap_q(const d2d_filter_def& f, int j) {
    const int h = f.ntaps / 2;
    return j >= h ? f.half[j - h] : f.half[h - 1 - j];
}
// full 32-bit tap j (0..N-1) of the 2^-(S+8) grid (filters/filter_tables.inc: half32), stored like the 24-bit halves
inline int64_t tap_q32(const d2d_filter_def& f, int j) {
    const int h = f.ntaps / 2;
    return j >= h ? f.half32[j - h] : f.half32[h - 1 - j];
}

// balanced base-256 digit l of v (the int8 limbs of a tap): v = d0 + d1*2^8 + d2*2^16 + d3*2^24, every d in [-128, 127]
inline int8_t limb256(int64_t v, int l) {
    int8_t dgt = 0;
    for (int i = 0; i <= l; ++i) {
        int64_t dd = ((v + 128) & 255) - 128;
        dgt = (int8_t)dd;
        v = (v - dd) / 256;
    }
    return dgt;
}

struct MfmaLayout {
    int M = 0, N = 0;
    int ksteps = 0;       // K steps of 32 bits over the widened window
    int phases = 8;       // output phases per matrix row
    int limbs = 4;        // int8 limbs per 32-bit tap
};
inline MfmaLayout mfma_layout(int M, int N) {
    MfmaLayout g;
    g.M = M; g.N = N;
    const int wd = (N + 7 * M + 24 + 31) / 32;   // dwords of one row's window (+ up to 3 bytes of misalignment)
    const int U = (wd + 1) / 2;
    g.ksteps = 2 * U;
    return g;
}
inline int mfma2_pairs(int M, int N) { return (N + 7 * M + 24 + 63) / 64; }   // two-group kernels: pair steps of a group's window
// plane 0 unmasked: a byte then weighs up to 128*128 + 254*128 in a limb sum; the int32 recombination needs the sums below 2^23
__host__ __device__ constexpr bool m2_unmask0(int NPG) { return (long long)NPG * 8 * (128 * 128 + 254 * 128) < (1 << 23); }
// stage B (d2d_kernels_rs.hip): bytes between two rows of a limb plane: the samples a row needs (P + 146) rounded up to 16, plus 16 or 32
// so that the pitch is an ODD number of 16-byte slots (the 64 lanes' 16-byte reads then fall on all banks)
__host__ __device__ constexpr int rs2_rp(int P) { return 16 * ((P + 146 + 15) / 16 + (((P + 146 + 15) / 16) % 2 ? 2 : 1)); }
uint32_t resamp2_nstep(const d2d_resamp_def& r);

uint64_t sum_abs_q(const d2d_filter_def& f);       // sum |q_j| of the tap table (bounds |y*2^S|)
uint64_t max_phase_sum_abs(const d2d_poly_def& p); // the largest per-phase sum |Q| of a composed table
bool mx_exact(const d2d_filter_def& f);            // do the digit sums of this table recombine exactly in f32?
bool mx_wide_exact(const d2d_filter_def& f);       // ... and do the seven digit sums of its half32 taps recombine exactly?
bool px_exact(const d2d_poly_def& p);              // do the composed table's base-32 digit sums recombine exactly in f32?

// tap_bits = 32 in two passes: the residual table q32 - 256 q as a filter of its own; `storage` holds its half
d2d_filter_def residual_def(const d2d_filter_def& f, std::vector<int32_t>& storage);

std::vector<double> build_lut_tables(const d2d_filter_def& f, int MB, bool msb_first);
std::vector<int8_t> build_mfma_tables(const d2d_filter_def& f, const MfmaLayout& g, bool msb_first);
// `unmask0`: plane 0 of a stream dword reaches the matrix cores unmasked where the limb sums allow it (two-group kernel); false: all masked (pipelined)
std::vector<int8_t> build_mfma2_tables(const d2d_filter_def& f, bool msb_first, bool unmask0);
std::vector<int8_t> build_mx_tables(const d2d_filter_def& f, bool msb_first, bool wide = false);   // wide: the 32-bit taps (f.half32)
std::vector<int8_t> build_px_tables(const d2d_poly_def& p);
std::vector<int8_t> build_resamp2_table(const d2d_resamp_def& r);
// an engine's matrix-core FIR table: fp6 digits for PIPE_FP6, else two-group fragments (masked under a pipelined kernel), else one-group ones
std::vector<int8_t> build_fir_table(const d2d_filter_def& f, int pipe, bool two_group, const MfmaLayout& layout, bool msb_first, bool wide);

}  // namespace d2d
