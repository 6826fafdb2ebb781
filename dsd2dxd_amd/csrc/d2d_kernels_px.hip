// d2d_kernels_px.hip -- DSD64 / DSD128 -> 96 / 192 / 384 kHz and DSD256 -> 192 / 384 kHz in ONE pass over the packed bits (gfx950), exact.
//
// The reference documents these rates as "cascaded FIR filters" (README.md:230, src/main.rs:88-89); until round 3 this engine ran them as
// two kernels that met in HBM (a decimator to 352.8 kHz writing int32, a polyphase L/147 resampler reading them back: 5.7 x the
// algorithmic traffic at DSD64 -> 96 kHz).  Here the two designs are composed into one polyphase filter on the bits (tools/design_filters.py:
// compose_polyphase),
//
//     y[m] = sum_j c[rho][j] s[q + D - j],   Mp m = Lp q + rho,   c = Q 2^-S,
//
// which is the decimators' arithmetic with a tap set per phase rho and windows that start at ANY bit: v = sum Q s is an exact integer
// (|v| < 2^31), y = v 2^-S, then level / dither / requantise as everywhere else.
//
//   d2d_fir_px_kernel<LP, MP, NP, G, KIND>   the fp6 x fp4 matrix-core form (v_mfma_scale_f32_32x32x64_f8f6f4, as d2d_kernels_mx.hip):
//       B operand = the bit stream, one nibble per bit (five vector instructions per 32 bits), A operand = the taps in five balanced
//       base-32 digits (e2m3), f32 accumulators holding exact digit sums.  Matrix row = (output of a GROUP of five, digit): 25 of 32
//       rows; a lane half owns outputs 0-2 / 3-4 of every group with all five digits of a sample in its own registers.  Matrix column
//       = G consecutive groups, a whole number of the filter's cycles, so every column sees the same taps at the same places; its
//       window starts at an arbitrary BIT of the stream: the lane reads the two dwords around it and one v_alignbit_b32 lines the
//       column up (the staged image is in time order, LSB first: MSB-first streams are bit-reversed per byte while they are staged).
//       Every (step, group) pair has its own tap fragment (the groups are 147 / 73.5 / 36.75 bits apart: no two share one).
//   d2d_poly_plain_kernel                    the same sums bit by bit, one output per lane: what D2D_KERNEL_LUT engines run at these rates
//                                            and the cross-check of the matrix-core form in every parity test.
//
// Replaces: the 48 kHz-family path inside Rdsd2Pcm::do_conversion (/root/reference/src/main.rs:345,429); the crate that holds it is
// absent from the reference.
#include <array>

#include "d2d_px_kernel.h"
#include "d2d_route.h"

namespace d2d {

// This object is unit 0 of D2D_PX_UNIT_LIST and holds the plain kernel and the dispatcher (the table builder: d2d_tables.cpp).
#define X(unit, lp, mp, np, g) +1
static_assert(D2D_PX_UNITS == 0 D2D_PX_UNIT_LIST(X), "the Makefile's PX_UNITS is not the length of D2D_PX_UNIT_LIST (d2d_px.h)");
#undef X
#define X(unit, lp, mp, np, g) extern template hipError_t launch_px_unit<unit>(const FirLaunch& p, uint32_t max_nout, uint32_t nfiles, hipStream_t s);
D2D_PX_UNIT_LIST(X)
#undef X
template hipError_t launch_px_unit<0>(const FirLaunch& p, uint32_t max_nout, uint32_t nfiles, hipStream_t s);

// one launcher per unit number; which unit serves a table: d2d_route.cpp
static const std::array<FirLauncher*, D2D_PX_UNITS> px_launchers = [] {
    std::array<FirLauncher*, D2D_PX_UNITS> v{};
#define X(unit, lp, mp, np, g) std::get<unit>(v) = &launch_px_unit<unit>;
    D2D_PX_UNIT_LIST(X)
#undef X
    return v;
}();

// ---- the plain form: one output per lane, bit by bit ----
__global__ __launch_bounds__(PXP_THREADS) void d2d_poly_plain_kernel(PxArgs a, uint32_t span) {
    extern __shared__ __align__(16) unsigned char smem[];
    int32_t* tq = reinterpret_cast<int32_t*>(smem);                                  // Q[Lp][NP]
    double* red = reinterpret_cast<double*>(smem + (((size_t)a.Lp * a.NP * 4 + 15) & ~(size_t)15));
    uint8_t* win = reinterpret_cast<uint8_t*>(red + 4);
    const StreamJob job = a.jobs[blockIdx.y];
    const uint32_t tid = threadIdx.x;
    for (uint32_t i = tid; i < a.Lp * a.NP; i += PXP_THREADS) tq[i] = reinterpret_cast<const int32_t*>(a.tables)[i];
    const uint32_t ntiles = (job.nout + PXP_THREADS - 1) / PXP_THREADS;
    const uint32_t sample_bytes = a.epi.sample_bytes, frame_bytes = sample_bytes * a.epi.channels;
    double pk = 0.0;
    for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint64_t mt = job.n0 + (uint64_t)tile * PXP_THREADS;
        // the tile's oldest bit: the first output's window start, call-relative
        const int64_t first_bit = (int64_t)(mt * a.Mp / a.Lp) + a.D - (int64_t)(a.NP - 1) - 8 * job.e0;
        const int64_t abeg = (first_bit >> 3) & ~(int64_t)15;
        __syncthreads();
        stage_window(win, job, a.in_channels, a.B, a.keep, abeg, span, tid, PXP_THREADS);
        __syncthreads();
        const uint32_t nl = tile * PXP_THREADS + tid;
        if (nl >= job.nout) continue;
        const uint64_t m = job.n0 + nl;
        const uint64_t tt = m * a.Mp;
        const int64_t q = (int64_t)(tt / a.Lp);
        const uint32_t rho = (uint32_t)(tt % a.Lp);
        const int32_t* g = tq + (size_t)rho * a.NP;
        const int32_t b0 = (int32_t)(q + a.D - 8 * job.e0 - 8 * abeg);             // the newest bit, relative to the staged window
        int64_t acc = 0;
        for (uint32_t j = 0; j < a.NP; ++j) {
            const uint32_t b = (uint32_t)(b0 - (int32_t)j);
            const uint32_t byte = win[b >> 3];
            const uint32_t bit = a.msb ? (byte >> (7u - (b & 7u))) & 1u : (byte >> (b & 7u)) & 1u;
            acc += bit ? (int64_t)g[j] : -(int64_t)g[j];
        }
        if (a.to_scratch) {
            job.xs[nl] = (int32_t)acc;
        } else {
            uint8_t* dst = reinterpret_cast<uint8_t*>(job.out) + (size_t)nl * frame_bytes + job.och * sample_bytes;
            pk = fmax(pk, emit_sample(a.epi, job, ldexp((double)acc, -a.S), m, dst));
        }
    }
    if (!a.to_scratch) block_peak_max(pk, job.peak, red);
}

// (the arguments, the span of a tile's windows and the LDS bytes: d2d_route.cpp, px_plan)
hipError_t launch_poly_plain(const FirLaunch& p, uint32_t max_nout, uint32_t nfiles, hipStream_t s) {
    const uint32_t nstreams = nfiles * p.rows_per_file;
    if (max_nout == 0 || nstreams == 0) return hipSuccess;
    static KernelPrep prep;
    hipError_t e = prep.max_dynamic_lds(reinterpret_cast<const void*>(&d2d_poly_plain_kernel), 160 * 1024);
    if (e != hipSuccess) return e;
    const uint32_t ntiles = (max_nout + p.tile - 1) / p.tile;
    const uint32_t gx = std::min(ntiles, std::max(1u, 2048u / nstreams));
    hipLaunchKernelGGL(d2d_poly_plain_kernel, dim3(gx, nstreams), dim3(PXP_THREADS), p.lds, s, p.px, p.px_span);
    d2d_last_launched_kernel = "d2d_poly_plain_kernel";
    return hipGetLastError();
}

hipError_t launch_fir_px(const FirLaunch& p, uint32_t max_nout, uint32_t nfiles, hipStream_t s) {
    if (max_nout == 0 || nfiles == 0) return hipSuccess;
    return p.unit >= 0 ? px_launchers[p.unit](p, max_nout, nfiles, s) : hipErrorInvalidValue;
}

}  // namespace d2d
