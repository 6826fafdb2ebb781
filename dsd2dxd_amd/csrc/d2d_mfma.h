// d2d_mfma.h -- the int8-MFMA FIR kernels (d2d_kernels_mfma*.hip) as host and device both see them: launch arguments, staging geometry
// (the tables: d2d_tables.h; which kernel serves an engine, and the arguments' values: d2d_route.h)
#pragma once
#include <hip/hip_runtime.h>

#include "d2d_tables.h"

namespace d2d {

// Diagnostics (phase ablations, in-kernel cycle stamps, start staggering, the MFMA-phase token) exist
// only in a build with -DD2D_DIAG=1 (make DIAG=1); the production kernel carries none of their state.
#ifndef D2D_DIAG
#define D2D_DIAG 0
#endif

struct MfmaArgs {
    FirArgs f;
    double c1, c0;        // x = fma(acc128, c1, -c0) == round(y*c0): c1 = 2^(1-S-7)*c0, c0 = scale | gain | 1
    // integer-depth epilogue as data: d = fma(term, dmul, dadd), clamp to [qmin_i, qmax_i], << qsh
    double dmul, dadd;
    uint32_t dsel;        // 1: triangular term, 0: rectangular term
    uint32_t dkind;       // 0: no dither, 1: triangular, 2: rectangular (chooses the register epilogue's instantiation)
    uint32_t qsh;         // 4 for 20-bit samples in a 24-bit container, else 0
    int32_t qmin_i, qmax_i;
    uint32_t wide;        // 1: limb sums may exceed 2^23, recombine in f64
    uint32_t U;           // dwords of row window per lane half; K steps = 2U
    uint32_t span;        // logical staged bytes per channel (multiple of 16)
    uint32_t ppair;       // physical LDS bytes per channel PAIR (dword-interleaved, padded rows)
    uint32_t ls;          // log2(row stride in dwords) = log2(2*MB)
    uint32_t off_waves;   // LDS: start of the per-wave regions (after the shared tap table)
    uint32_t wave_lds;    // LDS bytes per wave
    uint32_t off_out, off_pk;   // inside a wave's region
    uint32_t nwaves;      // waves per block
    uint32_t ngroups;     // channel groups per file: 1 for mono/stereo, else one block column per channel PAIR
    uint32_t dbg;         // diagnostic ablation mask (env D2D_DBG), 0 in production
    uint32_t stagger;     // start offset between wave slots, in units of 1024 cycles
};

void mfma_debug_stamps(unsigned long long out[8]);   // diagnostic (D2D_DBG=16)

// second-generation kernel (d2d_kernels_mfma2.hip): two phase groups per matrix column; its pipelined variants (d2d_kernels_mfma3.hip,
// d2d_kernels_mx.hip) take the same arguments
struct Mfma2Args {
    FirArgs f;
    double c1, c0;        // x = fma(acc128, c1, -c0) == round(y*c0): c1 = 2^(1-S-7)*c0, c0 = scale | gain | 2^S
    double dmul, dadd;    // integer depths: d = fma(term, dmul, dadd)
    uint32_t dkind;       // 0: no dither, 1: triangular, 2: rectangular
    uint32_t qsh;         // 4 for 20-bit samples in a 24-bit container, else 0
    int32_t qmin_i, qmax_i;
    uint32_t wide;        // 1: limb sums may exceed 2^23, recombine in f64
    uint32_t off_waves;   // LDS: start of the per-wave regions (after the shared tap table)
    uint32_t wave_lds;    // LDS bytes per wave
    uint32_t off_out;     // the wave's output slice inside its region
    uint32_t nwaves;      // waves per block
    uint32_t ngroups;     // channel groups per file: 1 for mono/stereo, else one block row per channel PAIR
    uint32_t intq;        // 1: unit gain at an integer depth -- the all-integer requantiser applies
    uint32_t gainq;       // 1 (pipelined kernels): another level in dB -- the f64 requantiser inside the pipelined epilogue (KIND + 4)
    int32_t  fbits;       // intq: x = v * 2^-fbits LSB (v = sum q s), fbits = S - (bits - 1)
    uint32_t dbg;         // diagnostic ablation mask (make DIAG=1, env D2D_DBG): 1 no chain, 2 no epilogue, 4 no staging
    uint32_t npairs;      // fp6 kernel: channel pairs a wave converts per tile (1; 3: planar 5.1 frames -- whole frames from one wave, one block row per file)
};

constexpr int M2_TILE = 512;          // outputs per wave-tile and channel

// staged dword L lives at L + (L >> m2_lsh(MB)): one pad dword per row stride of 4 MB dwords
__host__ __device__ constexpr int m2_lsh(int MB) { return MB == 1 ? 2 : MB == 2 ? 3 : MB == 4 ? 4 : MB == 8 ? 5 : 6; }
__host__ __device__ constexpr int m2_span_dw(int MB, int NPG) { return 31 * 4 * MB + 2 * (NPG + MB); }
__host__ __device__ constexpr int m2_chunks(int MB, int NPG) { return (m2_span_dw(MB, NPG) + 3 + 3) / 4; }   // + up to 3 dwords in front
__host__ __device__ constexpr int m2_pf(int MB, int NPG) { return (m2_chunks(MB, NPG) + 63) / 64; }
__host__ __device__ constexpr int m2_stream_bytes(int MB, int NPG) {
    const int dw = 4 * 64 * m2_pf(MB, NPG);
    return (((dw + (dw >> m2_lsh(MB)) + 4) * 4 + 15) & ~15) + 16;   // + a dummy slot for the dwords in front of the window
}

// (MB, NPG) pairs with a compiled two-group kernel
// M = 32 and 64 only: with 1 or 2 bytes per output a 512-output tile holds so little stream that the per-tile work
// (staging, waits, the epilogue) outweighs the shorter chain and the one-group kernel is faster (measured: DSD64 -> 352.8 kHz
// float 451 against 514 Gsamples/s, the M = 8 stage A of the 48k cascade 4.7 against 3.8 ms)
#define D2D_M2_SHAPES(X) X(4, 10) X(4, 12) X(4, 13) X(8, 19) X(8, 24) X(8, 25)

void mfma2_debug_stamps(unsigned long long out[8]);   // diagnostic (make DIAG=1, D2D_DBG & 256)
void mfma3_debug_stamps(unsigned long long out[8]);  // diagnostic (make DIAG=1, D2D_DBG & 256): per-wave lifetimes of the pipelined kernel

}  // namespace d2d
