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
#include <array>

#include "d2d_m3_kernel.h"
#include "d2d_route.h"

namespace d2d {

// ---- host side -------------------------------------------------------------------------------
// This object is unit 0 of D2D_M3_UNIT_LIST (the E_M8 shape) and holds the dispatcher.  (The tap tables are the two-group kernel's:
// build_mfma2_tables in d2d_tables.cpp, every plane masked.)
#define X(unit, mb, npg, nt0, nt1) +1
static_assert(D2D_M3_UNITS == 0 D2D_M3_UNIT_LIST(X), "the Makefile's M3_UNITS is not the length of D2D_M3_UNIT_LIST (d2d_m3.h)");
#undef X
#define X(unit, mb, npg, nt0, nt1) extern template hipError_t launch_m3_unit<unit>(const FirLaunch& p, uint32_t max_nout, uint32_t nfiles, hipStream_t s);
D2D_M3_UNIT_LIST(X)
#undef X
template hipError_t launch_m3_unit<0>(const FirLaunch& p, uint32_t max_nout, uint32_t nfiles, hipStream_t s);

// one launcher per unit number (null: a unit an A/B build leaves out); which unit serves a shape: d2d_route.cpp
static const std::array<FirLauncher*, D2D_M3_UNITS> m3_launchers = [] {
    std::array<FirLauncher*, D2D_M3_UNITS> v{};
#define X(unit, mb, npg, nt0, nt1) if constexpr (m3_unit_kept(mb, npg)) std::get<unit>(v) = &launch_m3_unit<unit>;
    D2D_M3_UNIT_LIST(X)
#undef X
    return v;
}();

hipError_t launch_fir_mfma3(const FirLaunch& p, uint32_t max_nout, uint32_t nfiles, hipStream_t s) {
    if (nfiles == 0 || max_nout == 0) return hipSuccess;
    return p.unit >= 0 && m3_launchers[p.unit] ? m3_launchers[p.unit](p, max_nout, nfiles, s) : hipErrorInvalidValue;
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
