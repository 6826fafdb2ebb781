// d2d_route.h -- which kernel, which tap-table layout and which staging serve an engine, decided once (choose_route), and everything those
// decisions read: the lookups in the lists of compiled kernels, the matrix-core kernels' launch geometry, the FIR launch arguments.  The unit
// (d2d_route.cpp) calls no HIP function: tools/route_probe.cpp builds from it and d2d_tables.cpp with g++ alone and prints the route of every
// configuration, which tests/golden/route_predicates.json and tests/golden/route_matrix.json pin (tests/test_route_cpu.py).
#pragma once
#include <string>

#include "d2d_m3.h"
#include "d2d_mfma.h"

namespace d2d {

// ---- the compiled kernels: the unit of D2D_MX_UNIT_LIST / D2D_M3_UNIT_LIST / D2D_PX_UNIT_LIST that serves a shape, or -1 (the dispatchers hold
// one launcher per unit number)
int mx_find(int MB, int NT, MxFlavour fl, int npr);
int m3_find(int MB, int NPG);
bool m3_frames(int unit, int NT);                  // does that unit serve frames with NT taps?
int px_find(const d2d_poly_def& p);
bool mfma_supported(int M, int N);
bool mfma2_supported(int M, int N);

// ---- launch geometry ----
void mfma_geometry(const FirArgs& a, const MfmaLayout& g, MfmaArgs& m, size_t& smem);
size_t mfma_smem_bytes(const MfmaLayout& g, uint32_t channels, uint32_t sample_bytes, uint32_t* waves_per_block);
void mfma2_geometry(const FirArgs& a, int MB, int NPG, Mfma2Args& m, size_t& smem);
size_t mfma2_smem_bytes(int M, int N, uint32_t channels, uint32_t sample_bytes, uint32_t* waves_per_block);
int mfma2_epilogue(const FirArgs& a, const Mfma2Args& m);
// does this launch shape go to a software-pipelined kernel?  Fixed per engine: decides the table variant.  A PipeKind.
int mfma2_pipelined(const FirArgs& a, int M, int N);
// the arguments of a two-group launch as the kernel that serves it wants them (launch_fir_mfma2)
void mfma2_launch_args(const FirArgs& a, int MB, int NPG, int N, Mfma2Args& m, size_t& smem);
int mx_launch_unit(const Mfma2Args& m, int MB, int NT);      // the fp6 kernel's unit for a launch (launch_fir_mx), or -1

// ---- the route of an engine ----
struct FirRoute {
    uint32_t kernel = D2D_KERNEL_LUT;
    bool poly = false;                    // DSD64 / DSD128 -> 48k multiples: one polyphase pass over the bits (d2d_kernels_px.hip)
    bool poly_plain = false;              // ... through the bit-by-bit kernel (D2D_KERNEL_LUT engines)
    bool mfma_v2 = false;                 // the two-group matrix-core kernel (d2d_kernels_mfma2.hip) serves this shape
    int mfma_pipe = PIPE_NONE;            // ... through a software-pipelined variant: PIPE_INT8 (d2d_kernels_mfma3.hip) or PIPE_FP6 (d2d_kernels_mx.hip)
    int mfma_pipe_lo = PIPE_NONE;         // ... and the residual table's pass (fine)
    // tap_bits = 32: the FIR runs twice into the scratch (the 24-bit table, then the residual table q32 - 256 q) and d2d_fine_combine_kernel
    // finishes v = 256 v_hi + v_lo
    bool fine = false;
    bool taps32 = false;                  // tap_bits = 32 in ONE pass: stereo at M = 32 on the fp6 kernel's seven-digit flavour -- one table, no scratch, no combining pass
    bool deinterleave = false;            // byte-interleaved input: a planar copy is made per call (d2d_deinterleave_kernel)
    bool il2 = false;                     // byte-interleaved stereo input de-interleaved inside the pipelined frame kernels' staging (FirArgs::il2)
    bool coop = false;                    // byte-interleaved 4/8-channel input de-interleaved inside the fp6 kernel's staging (FirArgs::coop)
    uint32_t B = 1;                       // effective block size of the layout the FIR kernels read
    uint32_t keep = 0;                    // history bytes per channel
    // MONO2: a mono stream on a pipelined kernel as a planar PAIR -- the two halves of a call converted side by side (FirArgs::mono2).
    // PIPE_FP6: the fp6 kernel (M = 32, 64, 128), PIPE_INT8: the int8 pipelined kernel (M = 8, 16), PIPE_NONE: no pair
    int mono2_pipe = PIPE_NONE;
    uint32_t table_variant = 0;           // TableBlobHeader::table_variant
};

// How to turn an f64 sample into output bytes, from the parameters ('N' at 32 bits is 'X': float output, nothing to shape; else 'N' stays and
// the FIR writes integers that a sequential pass requantises).
Epilogue epilogue_of(const d2d_params& p);
// Every choice of d2d_create, in its order.  D2D_OK, or the error of a configuration nothing serves with its text in `err`.
int choose_route(const d2d_params& p, const FilterChoice& fc, FirRoute& r, std::string& err);
uint32_t route_table_variant(const FirRoute& r);
// The part of a FIR launch's arguments that is fixed when the engine is created (`tables` and `jobs`: the engine's, filled in afterwards).
// `lo`: the residual table's pass.  choose_route also calls it on the half-chosen route, to ask mfma2_pipelined what would serve a format.
FirArgs fir_args_static(const d2d_params& p, const FilterChoice& fc, const Epilogue& epi, const FirRoute& r, const d2d_filter_def* lo = nullptr);
// the FIR kernel the dispatch will choose, spelled the way rocprofv3 prints it (d2d_kernel_name before the first call)
std::string route_kernel_name(const FirRoute& r, const FilterChoice& fc, const Epilogue& epi);

}  // namespace d2d
