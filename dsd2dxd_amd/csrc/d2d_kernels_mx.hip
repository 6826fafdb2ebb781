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
#include <array>

#include "d2d_mx_kernel.h"
#include "d2d_route.h"

namespace d2d {

// ---- host side -------------------------------------------------------------------------------
// This object is unit 0 of D2D_MX_UNIT_LIST (the E_M32 shape's integer kernels) and holds the dispatcher (the table builder: d2d_tables.cpp).
#define X(unit, mb, nt, fl, npr) +1
static_assert(D2D_MX_UNITS == 0 D2D_MX_UNIT_LIST(X), "the Makefile's MX_UNITS is not the length of D2D_MX_UNIT_LIST (d2d_mx.h)");
#undef X
#define X(unit, mb, nt, fl, npr) extern template hipError_t launch_mx_unit<unit>(const FirLaunch& p, uint32_t max_nout, uint32_t nfiles, hipStream_t s);
D2D_MX_UNIT_LIST(X)
#undef X
template hipError_t launch_mx_unit<0>(const FirLaunch& p, uint32_t max_nout, uint32_t nfiles, hipStream_t s);

// one launcher per unit number (null: a unit an A/B build leaves out); which unit serves a launch: d2d_route.cpp
static const std::array<FirLauncher*, D2D_MX_UNITS> mx_launchers = [] {
    std::array<FirLauncher*, D2D_MX_UNITS> v{};
#define X(unit, mb, nt, fl, npr) if constexpr (mx_unit_kept(mb, nt)) std::get<unit>(v) = &launch_mx_unit<unit>;
    D2D_MX_UNIT_LIST(X)
#undef X
    return v;
}();

hipError_t launch_fir_mx(const FirLaunch& p, uint32_t max_nout, uint32_t nfiles, hipStream_t s) {
    if (nfiles == 0 || max_nout == 0) return hipSuccess;
    return p.unit >= 0 && mx_launchers[p.unit] ? mx_launchers[p.unit](p, max_nout, nfiles, s) : hipErrorInvalidValue;
}
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
