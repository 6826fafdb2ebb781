// d2d_mix.hip -- the mix pass of a mixed engine (d2d_create_mix).
//
// The FIR kernels have written every input channel's exact integer sums x_c into its scratch line (their to_scratch form, as for the 'N'
// dither).  This pass turns a file's C lines into frames of Co channels: v_o = sum_c m[o][c] x_c in int64, y_o = (double)v_o * 2^-(S+15),
// then level, dither of OUTPUT channel o, requantisation and packing through emit_sample (d2d_device.h) -- mix/d2d_mix.h has the contract.
//
// Modelled on d2d_fine_combine_kernel (d2d_kernels.hip): a block takes 256 K frames of one file; a thread reads its frames' C integers
// (a channel's reads are consecutive across the block), the matrix sits in LDS and every lane reads the same word of it at a time (a
// broadcast, no bank conflict), the frames meet in an LDS image and leave as 16-byte stores; the peaks of an output channel are reduced per
// wave, then per block in LDS, then one atomic per block.  Job row f C + o serves output channel o: its dither keys are channel o's
// (the engine refuses a channel subset with a mix), its peak slot is d2d_peak's (file, o).
#include <hip/hip_runtime.h>

#include "../d2d_device.h"
#include "../d2d_launch.h"
#include "d2d_mix.h"

namespace d2d {

constexpr uint32_t MIX_FRAMES = 256;

template <int K, int CMAX>        // K chunks of 256 frames per trip (their scratch reads are all requested before the first is used), at most CMAX input channels
__global__ __launch_bounds__(MIX_FRAMES) void d2d_mix_kernel(const StreamJob* jobs, const int32_t* mix, uint32_t C, int sbits, Epilogue epi) {
    extern __shared__ __align__(16) uint8_t mix_lds[];                   // [Co x C coefficients, padded to 16 bytes][the frame image]
    __shared__ unsigned long long pkl[MIX_MAX_CHANNELS];                 // per output channel: the block's peak (non-negative doubles order like their bits)
    const uint32_t Co = epi.channels, sb = epi.sample_bytes, fb = Co * sb;
    const StreamJob* fj = jobs + (size_t)blockIdx.y * C;
    const uint32_t nout = fj[0].nout;
    int32_t* ml = reinterpret_cast<int32_t*>(mix_lds);
    uint8_t* img = mix_lds + ((Co * C * 4u + 15u) & ~15u);
    for (uint32_t i = threadIdx.x; i < Co * C; i += MIX_FRAMES) ml[i] = mix[i];
    if (threadIdx.x < MIX_MAX_CHANNELS) pkl[threadIdx.x] = 0ull;
    __syncthreads();
    const double ys = ldexp(1.0, -sbits);
    constexpr uint32_t SPAN = MIX_FRAMES * K;
    for (uint32_t n0 = blockIdx.x * SPAN; n0 < nout; n0 += gridDim.x * SPAN) {      // (block-uniform)
        int32_t x[K][CMAX];
#pragma unroll
        for (int c = 0; c < CMAX; ++c) {
            if ((uint32_t)c < C) {
                const D2D_GLOBAL int32_t* xs = as_global(fj[c].xs);
#pragma unroll
                for (int k = 0; k < K; ++k) x[k][c] = xs[min(n0 + threadIdx.x + MIX_FRAMES * k, nout - 1u)];
            } else {
#pragma unroll
                for (int k = 0; k < K; ++k) x[k][c] = 0;
            }
        }
        for (uint32_t o = 0; o < Co; ++o) {
            const StreamJob& job = fj[o];                                 // (Co <= C: the row exists)
            const int32_t* row = ml + o * C;
            long long v[K];
#pragma unroll
            for (int k = 0; k < K; ++k) v[k] = 0;
#pragma unroll
            for (int c = 0; c < CMAX; ++c)
                if ((uint32_t)c < C) {
                    const long long m = row[c];
#pragma unroll
                    for (int k = 0; k < K; ++k) v[k] += m * (long long)x[k][c];
                }
            double pk = 0.0;
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const uint32_t fr = threadIdx.x + MIX_FRAMES * k, n = n0 + fr;
                if (n < nout) pk = fmax(pk, emit_sample(epi, job, mix_value(v[k], ys), job.n0 + n, img + fr * fb + o * sb));
            }
#pragma unroll
            for (int s = 32; s > 0; s >>= 1) pk = fmax(pk, __shfl_xor(pk, s));
            if ((threadIdx.x & 63) == 0 && pk > 0.0) atomicMax(&pkl[o], (unsigned long long)__double_as_longlong(pk));
        }
        __syncthreads();
        const uint32_t nbytes = min(SPAN, nout - n0) * fb;
        uint8_t* out = reinterpret_cast<uint8_t*>(fj[0].out) + (size_t)n0 * fb;     // 16-byte aligned: the buffer is, and 256 frames are a multiple of 16 bytes
        for (uint32_t i = 16u * threadIdx.x; i < nbytes; i += 16u * MIX_FRAMES) {
            if (i + 16u <= nbytes) *reinterpret_cast<D2D_GLOBAL u32x4*>(as_global(out + i)) = *reinterpret_cast<const u32x4*>(img + i);
            else for (uint32_t k = i; k < nbytes; ++k) out[k] = img[k];
        }
        __syncthreads();
    }
    if (threadIdx.x < Co && pkl[threadIdx.x]) atomicMax(reinterpret_cast<unsigned long long*>(fj[threadIdx.x].peak), pkl[threadIdx.x]);
}

template <int K, int CMAX>
static hipError_t launch_mix_t(const StreamJob* jobs, const int32_t* mix, uint32_t C, uint32_t nfiles, uint32_t max_nout, int sbits, const Epilogue& epi,
                               hipStream_t s) {
    const uint32_t span = MIX_FRAMES * (uint32_t)K;
    uint32_t gx = (max_nout + span - 1u) / span;
    const uint32_t cap = (8192u + nfiles - 1u) / nfiles;                            // about 8192 blocks in all, each walking its share of the chunks
    if (gx > cap) gx = cap;
    // the matrix (at most 64 x 64 x 4 = 16 KiB) and the frame image (at most 256 frames x 64 channels x 4 bytes = 64 KiB)
    const size_t smem = (((size_t)epi.channels * C * 4u + 15u) & ~(size_t)15) + (size_t)span * epi.channels * epi.sample_bytes;
    static KernelPrep prep;
    hipError_t e = prep.max_dynamic_lds(reinterpret_cast<const void*>(&d2d_mix_kernel<K, CMAX>), 96 * 1024);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((d2d_mix_kernel<K, CMAX>), dim3(gx, nfiles), dim3(MIX_FRAMES), smem, s, jobs, mix, C, sbits, epi);
    return hipGetLastError();
}

hipError_t launch_mix(const StreamJob* jobs, const int32_t* mix, uint32_t in_channels, uint32_t nfiles, uint32_t max_nout, int scale_bits,
                      const Epilogue& epi, hipStream_t s) {
    if (nfiles == 0 || max_nout == 0) return hipSuccess;
    if (in_channels < 1 || in_channels > MIX_MAX_CHANNELS || epi.channels < 1 || epi.channels > in_channels) return hipErrorInvalidValue;
    const int sbits = scale_bits + MIX_Q;
    if (in_channels <= 2) return launch_mix_t<4, 2>(jobs, mix, in_channels, nfiles, max_nout, sbits, epi, s);
    if (in_channels <= 8) return launch_mix_t<2, 8>(jobs, mix, in_channels, nfiles, max_nout, sbits, epi, s);
    return launch_mix_t<1, 64>(jobs, mix, in_channels, nfiles, max_nout, sbits, epi, s);
}

}  // namespace d2d
