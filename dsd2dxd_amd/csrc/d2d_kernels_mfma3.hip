// d2d_kernels_mfma3.hip -- the two-group int8 matrix-core FIR decimator, software-pipelined (gfx950), exact.
//
// Same arithmetic, tap tables, staging and output as d2d_kernels_mfma2.hip's stereo 24-bit flavour at 0 dB (EPI = 1 with
// the all-integer requantiser); what changes is WHEN a wave does the requantisation.  The two-group kernel alternates
// between a matrix-core chain and a vector-only epilogue, and with three waves per SIMD the two kinds of phase overlap
// only by chance (the parts of the kernel add up, profiles/r02_ablations.txt).  Here every chain carries the epilogue of
// the chain before it inside its own instruction stream:
//
//   region A (tile t):  chain of channel 0  ||  requantise channel 1 of tile t-1, then pack + store tile t-1
//   region B (tile t):  chain of channel 1  ||  requantise channel 0 of tile t
//
// so each wave keeps the matrix pipe and the vector issue port busy at the same time, whatever its neighbours do; two
// accumulator sets are live, the kernel runs two waves per SIMD (up to 256 VGPRs).  The epilogue interleaved with a chain
// is the branch-free fast form (whole tile, no clip possible, no exact rounding tie, dither counter not wrapping); a tile
// that fails one of those tests is redone after the region from its stream bytes, which are still in the wave's LDS buffer
// of that channel (one buffer per channel), by a plain chain and the general per-sample code -- identical results.
//
// The accumulators start from -2^S spread over the limb-3 rows (the MFMA's C operand) instead of zero, so a sample's limbs
// recombine to v = sum q s directly (no bias to carry through the epilogue), and the requantiser is
//   r = (v + (T >> (16 - F))) >> F,  T = lo16 + hi16 - 32767  (triangular; F = S - 23 fraction bits of x = v * 2^-F LSB)
// which is floor(x + d + 1/2) exactly: floor((a + y) / n) = floor((a + floor(y)) / n) for integers a, n.
//
// Replaces: the per-block translate loop inside Rdsd2Pcm::do_conversion
// (/root/reference/src/main.rs:345,429); the crate that holds it is absent from the reference.
#include <vector>

#include "d2d_m3_kernel.h"

namespace d2d {

// ---- host side -------------------------------------------------------------------------------
// This object is unit 0 of D2D_M3_UNIT_LIST (the E_M8 shape) and holds the dispatcher.  (The tap tables are the two-group kernel's:
// build_mfma2_tables in d2d_tables.cpp, every plane masked.)
#define X(unit, mb, npg, nt0, nt1) +1
static_assert(D2D_M3_UNITS == 0 D2D_M3_UNIT_LIST(X), "the Makefile's M3_UNITS is not the length of D2D_M3_UNIT_LIST (d2d_m3.h)");
#undef X
#define X(unit, mb, npg, nt0, nt1) extern template hipError_t launch_m3_unit<unit>(Mfma2Args& m, uint32_t nwt_max, uint32_t nrows, hipStream_t s);
D2D_M3_UNIT_LIST(X)
#undef X
template hipError_t launch_m3_unit<0>(Mfma2Args& m, uint32_t nwt_max, uint32_t nrows, hipStream_t s);

struct M3Row { int MB, NPG, nt[2]; hipError_t (*fn)(Mfma2Args&, uint32_t, uint32_t, hipStream_t); };
static const std::vector<M3Row>& m3_rows() {
    static const std::vector<M3Row> rows = [] {
        std::vector<M3Row> v;
#define X(unit, mb, npg, nt0, nt1) if constexpr (m3_unit_kept(mb, npg)) v.push_back({mb, npg, {nt0, nt1}, &launch_m3_unit<unit>});
        D2D_M3_UNIT_LIST(X)
#undef X
        return v;
    }();
    return rows;
}
// the row of a shape (one at most), and whether it serves frames with NT taps
static const M3Row* m3_find(int MB, int NPG) {
    for (const M3Row& r : m3_rows()) if (r.MB == MB && r.NPG == NPG) return &r;
    return nullptr;
}
static bool m3_frames(const M3Row* r, int NT) { return r && NT > 0 && (r->nt[0] == NT || r->nt[1] == NT); }
bool mfma3_scr_supported(int MB, int NPG) { return m3_find(MB, NPG) != nullptr; }
bool mfma3_supported(int MB, int NPG, int NT) { return m3_frames(m3_find(MB, NPG), NT); }

hipError_t launch_fir_mfma3(Mfma2Args& m, int MB, int NPG, int NT, uint32_t nwt_max, uint32_t nrows, hipStream_t s) {
    const M3Row* r = m3_find(MB, NPG);
    if (!r || (!m.f.to_scratch && !m3_frames(r, NT))) return hipErrorInvalidValue;
    return r->fn(m, nwt_max, nrows, s);
}

#if D2D_M3_STAMPS
void mfma3_debug_stamps(unsigned long long out[8]) {
    (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(d2d_m3_stamps), sizeof(unsigned long long) * 8);
    unsigned long long z[8] = {~0ull, 0, 0, 0, 0, 0, 0, 0};
    (void)hipMemcpyToSymbol(HIP_SYMBOL(d2d_m3_stamps), z, sizeof(z));
}
#else
void mfma3_debug_stamps(unsigned long long out[8]) { for (int i = 0; i < 8; ++i) out[i] = 0; }
#endif

}  // namespace d2d
