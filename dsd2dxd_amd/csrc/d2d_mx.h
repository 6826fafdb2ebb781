// d2d_mx.h -- geometry of the fp6 x fp4 matrix-core FIR kernel (d2d_kernels_mx.hip), shared by host and device.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "d2d_filters.h"
#include "d2d_internal.h"

namespace d2d {

constexpr int MX_FRAG_BYTES = 1536;          // a tap fragment: 64 lanes x 16 bytes, then 64 lanes x 8 bytes (32 e2m3 codes per lane)
#ifndef D2D_MX_THREADS
#define D2D_MX_THREADS 512     // waves per block x 64: 512 = two waves per SIMD (256 registers each); 768 = three (168), an A/B build
#endif

// MB = bytes per output (M / 8), NT = taps, G = groups of PH phases per matrix column.  PH = 6 with the 24-bit taps' five base-32 digits (30 of the
// 32 matrix rows), PH = 4 with the 32-bit taps' seven (28 rows; the one-pass form of tap_bits = 32, round 4)
__host__ __device__ constexpr int mx_cs(int MB, int G, int PH = 6) { return PH * G * MB / 4; }                 // column stride in dwords (PH G outputs)
__host__ __device__ constexpr int mx_dly(int MB, int PH = 6) { return PH * MB / 8; }                          // steps (64 bits) between two groups: PH M / 64
__host__ __device__ constexpr int mx_nf(int MB, int NT, int PH = 6) { return (NT + (PH - 1) * 8 * MB + 24 + 63) / 64; }   // fragments: window of PH phases + up to 3 bytes of misalignment
__host__ __device__ constexpr int mx_nstep(int MB, int NT, int G, int PH = 6) { return mx_nf(MB, NT, PH) + mx_dly(MB, PH) * (G - 1); }
__host__ __device__ constexpr int mx_span_dw(int MB, int NT, int G, int PH = 6) { return 31 * mx_cs(MB, G, PH) + 2 * mx_nstep(MB, NT, G, PH); }
__host__ __device__ constexpr int mx_chunks(int MB, int NT, int G, int PH = 6) { return (mx_span_dw(MB, NT, G, PH) + 3 + 3) / 4; }   // + up to 3 dwords in front
__host__ __device__ constexpr int mx_pf(int MB, int NT, int G, int PH = 6) { return (mx_chunks(MB, NT, G, PH) + 63) / 64; }
#ifndef D2D_MX_NOFLAT
#define D2D_MX_NOFLAT 0     // 1: the padded image for every shape (A/B builds)
#endif
#ifndef D2D_MX_FORCEFLAT
#define D2D_MX_FORCEFLAT 0  // 1: the unpadded image for every shape (A/B builds: bank conflicts on the window reads against fewer registers)
#endif
__host__ __device__ constexpr bool mx_flat(int MB, int G, int PH = 6) { return D2D_MX_FORCEFLAT || (!D2D_MX_NOFLAT && mx_cs(MB, G, PH) % 4 == 2); }        // unpadded LDS image (see the kernel)
__host__ __device__ constexpr int mx_stream_bytes(int MB, int NT, int G, int PH = 6) {
    const int dw = 4 * mx_chunks(MB, NT, G, PH);
    if (mx_flat(MB, G, PH)) return 4 * dw + 16;
    return (((dw + dw / mx_cs(MB, G, PH) + 4) * 4 + 15) & ~15) + 16;   // + a dummy slot for the dwords in front of the window
}

// index of the MFMA (step u, group g) among the MFMAs of a chain, in issue order
__host__ __device__ constexpr int mx_slot(int MB, int NT, int G, int u, int g, int PH = 6) {
    int k = 0;
    for (int uu = 0; uu <= u; ++uu)
        for (int gg = 0; gg < G; ++gg) {
            const int f = uu - mx_dly(MB, PH) * gg;
            if (f < 0 || f >= mx_nf(MB, NT, PH)) continue;
            if (uu == u && gg == g) return k;
            ++k;
        }
    return k;
}

// the first group with an MFMA at step u, and the MFMAs of the step
__host__ __device__ constexpr int mx_first_group(int MB, int NT, int u, int PH = 6) { return u < mx_nf(MB, NT, PH) ? 0 : (u - mx_nf(MB, NT, PH)) / mx_dly(MB, PH) + 1; }
__host__ __device__ constexpr int mx_step_mfmas(int MB, int NT, int G, int u, int PH = 6) {
    int n = 0;
    for (int g = 0; g < G; ++g) n += u - mx_dly(MB, PH) * g >= 0 && u - mx_dly(MB, PH) * g < mx_nf(MB, NT, PH) ? 1 : 0;
    return n;
}
// D2D_MX_FEED (below): the step behind whose first MFMA the B operand of step v > 0 is expanded -- the last one before v, at most two back, that has
// a second MFMA or a job riding on its first (NJ jobs over the chain's MFMAs, job j behind MFMA j NSLOT / NJ), so that something lies between the
// expansion and the MFMA that reads it
__host__ __device__ constexpr int mx_feed_step(int MB, int NT, int G, int v, int NJ, int PH = 6) {
    const int nslot = mx_nf(MB, NT, PH) * G;
    for (int u = v - 1; u >= 0 && u >= v - 2; --u) {
        if (mx_step_mfmas(MB, NT, G, u, PH) >= 2) return u;
        const int s = mx_slot(MB, NT, G, u, mx_first_group(MB, NT, u, PH), PH);
        for (int j = 0; j < NJ; ++j) if ((j * nslot) / NJ == s) return u;
    }
    return v - 1;
}

// groups per column: three at M = 32; at M = 64 the tap fragments of three groups do not fit the register file next to two accumulator sets
#ifndef D2D_MX_G4
#define D2D_MX_G4 3
#endif
#ifndef D2D_MX_G8
#define D2D_MX_G8 2
#endif
// M = 128: one group (the fragments of a second one would be held for twelve steps: 84 registers)
__host__ __device__ constexpr int mx_g(int MB) { return MB == 4 ? D2D_MX_G4 : MB == 16 ? 1 : D2D_MX_G8; }

// Resident tap fragments (M = 32: at most twelve fragments of six registers): a wave loads its variant of the table into registers at kernel entry
// and the chain reads no fragment from LDS.  D2D_MX_NRES < NF keeps only the first NRES there (the others come from LDS as everywhere else).
#ifndef D2D_MX_RESIDENT
#define D2D_MX_RESIDENT 1   // 0: no resident fragments anywhere (A/B builds)
#endif
#ifndef D2D_MX_NRES
#define D2D_MX_NRES 64
#endif
__host__ __device__ constexpr bool mx_resident(int MB, int NT, int PH = 6) { return D2D_MX_RESIDENT && MB == 4 && mx_nf(MB, NT, PH) <= 12; }
__host__ __device__ constexpr int mx_nres(int MB, int NT, int PH = 6) { return !mx_resident(MB, NT, PH) ? 0 : D2D_MX_NRES < mx_nf(MB, NT, PH) ? D2D_MX_NRES : mx_nf(MB, NT, PH); }
// Fragments a wave of one instantiation keeps in registers: the stereo frame flavours of the M = 32 rows.  The scratch flavour, several pairs
// per wave and the 32-bit taps read them from LDS like M = 64 and M = 128.
__host__ __device__ constexpr int mx_nres_of(int MB, int NT, int SBY, int NPR, int ND) { return SBY != 0 && NPR == 1 && ND == 5 ? mx_nres(MB, NT) : 0; }

// The resident dithered stereo flavours of the integer requantiser (KIND 1, 2: units 0-3) compile a second form that reads a call's dither words
// from a table (FirArgs::dither_words; d2d_mx_kernel.h: DT), taken by the calls whose files all start at one output index (d2d_engine.cpp:
// dither_table_serves).  The f64 requantiser's flavours (KIND 5-7) do not: they have no registers for words requested a region ahead, and with the
// words requested in the region that reads them a step was no faster than hashing (profiles/dither_table_check.md).  -DD2D_MX_DTAB=0 compiles the
// form out (A/B builds).
#ifndef D2D_MX_DTAB
#define D2D_MX_DTAB 1
#endif
#ifndef D2D_MX_DTAB_AHEAD
#define D2D_MX_DTAB_AHEAD 1 // the words are requested a region ahead of the epilogue that reads them, into two register sets; 0: in the same region, one set (measured: a third of the gain)
#endif
__host__ __device__ constexpr bool mx_dither_table(int MB, int NT, int KIND, int SBY, int NPR, int ND) {
    return D2D_MX_DTAB && NPR == 1 && (KIND == 1 || KIND == 2) && mx_nres_of(MB, NT, SBY, NPR, ND) > 0;
}

// Where the fragments are resident, the chain expands a step's B operand a step or two ahead, behind an earlier MFMA (d2d_mx_kernel.h: chain).
// -DD2D_MX_FEED=0: the resident flavours expand a step's B operand directly in front of its first MFMA, like the others (A/B builds)
#ifndef D2D_MX_FEED
#define D2D_MX_FEED 1
#endif

// ---- the compiled kernels: ONE row per object --------------------------------------------------------------------------------
// X(unit, MB, NT, flavour, NPR).  Unit n is d2d_mx_unit.hip compiled with -DD2D_MX_UNIT=n (unit 0 rides in d2d_kernels_mx.hip, next to the
// dispatcher) and holds every sample format of its row: launch_mx_unit in d2d_mx_kernel.h.  The dispatcher's table, the launch plan
// (d2d_route.cpp: mx_plan) and the mx_*_supported functions all read this list and nothing else.  Adding a shape is one row here plus MX_UNITS in the Makefile
// (the dispatcher's static_assert says so when the two disagree).
//   MX_INT   unit gain, all-integer requantiser (KIND 0-2: 24-bit, 16-bit, float frames); NPR = 1 also holds the exact integers for the scratch,
//            NPR > 1 converts that many channel pairs per wave (planar multichannel frames: 2 quad, 3 a 5.1 stream, 4 a 7.1 / eight-channel stream)
//   MX_GAIN  the f64 requantiser (KIND 4-7: other levels, 20-bit, the float dither) of the shapes that serve frames (not the cascade's A filters)
//   MX_WIDE  the one-pass form of the 32-bit tap grid (ND = 7, KIND 4-7; stereo frames)
// (MB, NT) are the filters X_M32, C_M32, E_M32, A_M32, A_M64, C_M64, E_M64, E_M128.
enum MxFlavour { MX_INT, MX_GAIN, MX_WIDE };
#define D2D_MX_UNIT_LIST(X)                                                                                              \
    X(0, 4, 560, MX_INT, 1)   X(1, 4, 352, MX_INT, 1)   X(2, 4, 384, MX_INT, 1)    X(3, 4, 512, MX_INT, 1)                  \
    X(4, 8, 688, MX_INT, 1)   X(5, 8, 1024, MX_INT, 1)  X(6, 8, 1104, MX_INT, 1)   X(7, 16, 2192, MX_INT, 1)                \
    X(8, 4, 560, MX_GAIN, 1)  X(9, 4, 384, MX_GAIN, 1)  X(10, 4, 512, MX_GAIN, 1)  X(11, 8, 1024, MX_GAIN, 1)               \
    X(12, 8, 1104, MX_GAIN, 1) X(13, 16, 2192, MX_GAIN, 1)                                                               \
    X(14, 4, 560, MX_INT, 3)  X(15, 8, 1104, MX_INT, 3) X(16, 16, 2192, MX_INT, 3) X(17, 4, 560, MX_INT, 2)                 \
    X(18, 4, 560, MX_INT, 4)  X(19, 8, 1104, MX_INT, 2) X(20, 8, 1104, MX_INT, 4)                                           \
    X(21, 4, 560, MX_WIDE, 1) X(22, 8, 1104, MX_WIDE, 1)
// -DD2D_MX_DEV (A/B builds, tools/ab_build.sh): only the rows of the E_M32 shape are in the table, so only their units need compiling
#ifdef D2D_MX_DEV
constexpr bool mx_unit_kept(int MB, int NT) { return MB == 4 && NT == 560; }
#else
constexpr bool mx_unit_kept(int, int) { return true; }
#endif

struct FirLaunch;
template <int UNIT> hipError_t launch_mx_unit(const FirLaunch& p, uint32_t max_nout, uint32_t nfiles, hipStream_t s);   // d2d_mx_kernel.h; one explicit instantiation per object
bool mx_supported(int MB, int NT);                 // is a kernel compiled for this shape?
bool mx_pairs_supported(int MB, int NT, int npairs);   // ... for `npairs` channel pairs per wave (planar multichannel frames)?
bool mx_gain_supported(int MB, int NT);            // ... and its gain flavours (frames at another level than 0 dB)?
bool mx_wide_supported(int MB, int NT);            // ... the one-pass form of the 32-bit tap grid (seven digits, four phases per group)?
int mx_groups(int MB);
void mx_debug_stamps(unsigned long long out[8]);   // diagnostic (-DD2D_MX_STAMPS=1 builds)

}  // namespace d2d
