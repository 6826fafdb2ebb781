// d2d_route.h -- which kernel, which tap-table layout and which staging serve an engine, decided once (choose_route), and everything those
// decisions read: the lookups in the lists of compiled kernels, and the plan of every FIR launch an engine can make (fir_launch: the instantiation,
// its arguments and its geometry).  The unit (d2d_route.cpp) calls no HIP function: tools/route_probe.cpp builds from it and d2d_tables.cpp with
// g++ alone and prints the route and the launches of every configuration, which tests/golden/route_*.json pin (tests/test_route_cpu.py).
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

// ---- the route of an engine ----
struct FirRoute {
    uint32_t kernel = D2D_KERNEL_LUT;
    bool poly = false;                    // filter E, DSD64 / DSD128 -> 48k multiples, DSD256 -> 192 / 384 kHz: one polyphase pass over the bits (d2d_kernels_px.hip)
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
// The parameters a MIXED engine's FIR pass is planned with (d2d_create_mix): the 'N' dither's integer pass of the same shape, so that every FIR
// kernel a mix can reach is one the noise shaper already reaches.  Float output plans as 24 bits ('N' at 32 bits would be 'X': frames).
d2d_params mix_fir_params(const d2d_params& p);
d2d_params half_fir_params(const d2d_params& p);      // ... and of a halved engine (d2d_create_half): the same at twice the output rate
// Every choice of d2d_create, in its order.  D2D_OK, or the error of a configuration nothing serves with its text in `err`.
int choose_route(const d2d_params& p, const FilterChoice& fc, FirRoute& r, std::string& err);
uint32_t route_table_variant(const FirRoute& r);
// The part of a FIR launch's arguments that is fixed when the engine is created (`tables` and `jobs`: the engine's, filled in afterwards).
// `lo`: the residual table's pass.  choose_route also calls it on the half-chosen route, to ask mfma2_pipelined what would serve a format.
FirArgs fir_args_static(const d2d_params& p, const FilterChoice& fc, const Epilogue& epi, const FirRoute& r, const d2d_filter_def* lo = nullptr);
// the FIR kernel the dispatch will choose, spelled the way rocprofv3 prints it (d2d_kernel_name before the first call)
std::string route_kernel_name(const FirRoute& r, const FilterChoice& fc, const Epilogue& epi);

// ---- the plan of a FIR launch: everything about it that no call changes, made once when the engine is created ----
enum FirFamily : int {
    FIR_LUT,                   // d2d_fir_lut_kernel<MB>
    FIR_MFMA,                  // d2d_fir_mfma_kernel<MB>                                  the one-group matrix-core kernel
    FIR_MFMA2,                 // d2d_fir_mfma2_kernel<MB, NPG, CH, EPI>                   the two-group one
    FIR_M3,                    // d2d_fir_mfma3_kernel<MB, NPG, NT, KIND, SBY>             pipelined, int8
    FIR_MX,                    // d2d_fir_mx_kernel<MB, NT, G, KIND, SBY, NPR, ND>         pipelined, fp6 x fp4
    FIR_PX,                    // d2d_fir_px_kernel<LP, MP, NP, G, KIND>                   the composed polyphase filter
    FIR_PX_PLAIN,              // d2d_poly_plain_kernel                                    ... bit by bit
};
struct FirLaunch {
    int family = FIR_LUT;
    // the object that holds the instantiation: the row of D2D_M3_UNIT_LIST / D2D_MX_UNIT_LIST / D2D_PX_UNIT_LIST or of D2D_M2_SHAPES, MB for
    // the LUT and one-group kernels, 0 for the plain one.  -1: no compiled kernel serves these arguments, the launcher returns hipErrorInvalidValue
    int unit = -1;
    int nt = 0, t[7] = {};     // the template arguments, in the order rocprofv3 prints them (the family's comment above)
    int kind() const { return family == FIR_PX ? t[4] : t[3]; }      // KIND, and for FIR_MFMA2 its EPI
    int sby() const { return t[4]; }                                  // SBY of the two pipelined kernels
    // the kernel's argument struct, whole; `jobs` and `tables` are the engine's (bind).  One of the three per family: m1 FIR_MFMA; px the two
    // polyphase kernels; m everything else (FIR_LUT passes m.f)
    MfmaArgs m1{};
    Mfma2Args m{};
    PxArgs px{};
    uint32_t px_span = 0;      // FIR_PX_PLAIN: bytes a tile's windows span (the kernel's second argument)
    size_t lds = 0;            // dynamic LDS bytes of a block
    uint32_t nwaves = 0;       // waves per block (FIR_MFMA2: what is asked for, the register file may admit fewer)
    uint32_t tile = 0;         // outputs per wave-tile (FIR_LUT, FIR_PX_PLAIN: per block)
    uint32_t block_tiles = 0;  // wave-tiles a block works on at a time: its waves, or one where the waves of a block share a tile (FirArgs::coop)
    uint32_t rows_per_file = 0;   // grid rows per file: channel groups, or one (coop, several pairs per wave), or streams (FIR_LUT, FIR_PX_PLAIN)
    std::string name;          // the kernel, spelled the way rocprofv3 prints it
    void bind(const StreamJob* jobs, const void* tables) { m1.f.jobs = m.f.jobs = px.jobs = jobs; m1.f.tables = m.f.tables = px.tables = tables; }
};
// The launches of an engine: its main pass (the composed polyphase pass where route.poly), the residual table's pass (route.fine; `lo` its
// filter) and the mono pair (route.mono2_pipe), on jobs of two "channels" per file.
enum FirPass { PASS_MAIN, PASS_LO, PASS_MONO2 };
FirLaunch fir_launch(const d2d_params& p, const FilterChoice& fc, const Epilogue& epi, const FirRoute& r, FirPass pass, const d2d_filter_def* lo = nullptr);

}  // namespace d2d
