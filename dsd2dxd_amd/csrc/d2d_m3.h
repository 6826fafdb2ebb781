// d2d_m3.h -- the compiled shapes of the pipelined int8 FIR kernel (d2d_kernels_mfma3.hip, d2d_m3_kernel.h) and its host entry points.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace d2d {

#define D2D_M3_THREADS 512
#ifndef D2D_M3_STAGED
#define D2D_M3_STAGED 1     // M = 8: a full tile's frames go through LDS and leave as aligned 1-KiB rows (0: straight from registers, A/B builds)
#endif

// ---- the compiled kernels: ONE row per object ---------------------------------------------------------------------------------
// X(unit, MB, NPG, NT0, NT1): MB = bytes per output (M / 8), NPG = pair steps of a group's window (mfma2_pairs(M, N) = (N + 7 M + 24 + 63) / 64).
// Unit n is d2d_m3_unit.hip compiled with -DD2D_M3_UNIT=n (unit 0 rides in d2d_kernels_mfma3.hip, next to the dispatcher) and holds every
// format of its row: launch_m3_unit in d2d_m3_kernel.h.  The dispatcher's table, the launch plan (d2d_route.cpp: m3_plan), mfma3_supported and
// mfma3_scr_supported all read this list and nothing else.  Adding a shape is one row here plus M3_UNITS in the Makefile (the
// dispatcher's static_assert says so when the two disagree).
//   every row   the exact integers for the scratch (the noise-shaping pass of the 44.1k-family filters, stage A of the 48k cascade)
//   NT0, NT1    the tap counts of that shape that serve stereo frames, 0 = none: 24-bit, 16-bit and float frames at 0 dB (KIND 0-2), and
//               for MB < 4 the f64 requantiser's flavours (KIND 4-7; M = 32 and 64 have them on the fp6 kernel).  A row without a tap count
//               compiles the scratch flavour only (the stage-A filters only ever write the scratch).
// The units' filters: 0 E_M8; 1 X_M8, D_M8, A_M8; 2 A_M16; 3 X_M16; 4 C_M16, E_M16; 5 X_M32, A_M32; 6 C_M32; 7 E_M32; 8 A_M64; 9 C_M64; 10 E_M64.
// (The M = 8 and 16 shapes are served by this kernel only: the two-group kernel loses to the one-group one there.)
#define D2D_M3_UNIT_LIST(X)                                                                                              \
    X(0, 1, 4, 144, 0)   X(1, 1, 3, 96, 0)     X(2, 2, 5, 0, 0)      X(3, 2, 6, 192, 0)    X(4, 2, 7, 256, 288)             \
    X(5, 4, 10, 384, 0)  X(6, 4, 12, 512, 0)   X(7, 4, 13, 560, 0)   X(8, 8, 19, 0, 0)     X(9, 8, 24, 1024, 0)             \
    X(10, 8, 25, 1104, 0)
// -DD2D_M3_DEV (A/B builds, tools/ab_build.sh): only unit 0's shape is in the table, so only d2d_kernels_mfma3.hip needs compiling
#ifdef D2D_M3_DEV
constexpr bool m3_unit_kept(int MB, int NPG) { return MB == 1 && NPG == 4; }
#else
constexpr bool m3_unit_kept(int, int) { return true; }
#endif

struct FirLaunch;
template <int UNIT> hipError_t launch_m3_unit(const FirLaunch& p, uint32_t max_nout, uint32_t nfiles, hipStream_t s);   // d2d_m3_kernel.h; one explicit instantiation per object
bool mfma3_supported(int MB, int NPG, int NT);     // is a kernel compiled that serves frames for this shape and tap count?
bool mfma3_scr_supported(int MB, int NPG);         // ... that writes the scratch for this shape?

}  // namespace d2d
