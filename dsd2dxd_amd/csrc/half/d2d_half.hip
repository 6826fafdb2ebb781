// d2d_half.hip -- the 2:1 decimator of a halved engine (d2d_create_half) and the pass on its own
// (d2d_half_frames_device).
//
// The FIR kernels have written every channel's exact integer sums x[i] into its scratch line (their to_scratch form, as for the 'N' dither),
// behind the HALF_HIST sums carried from the call before.  This pass makes the frames k with n0 <= 2k < n0 + nout:
// v = sum_j q[j] x[2k - j] in int64, w = (v + 2^(T-1)) >> T, y = (double)w * 2^-S, then level, dither of (channel, k), requantisation and
// packing through emit_sample (d2d_device.h) -- half/d2d_half.h has the contract.
//
// A block takes TILE = 4 x blockDim consecutive frames of one file and converts its channels one after the other.  For a channel it stages
// the 2 TILE + NT - 1 sums the tile reads into LDS, split into an even and an odd plane: with s[i] = x[2 k_first - (NT - 1) + i] frame t
// of the tile is sum_m qr[m] s[2t + m] (qr: the taps reversed), the even m walk E[t + a] = s[2(t + a)], the odd ones O[t + a].  A lane owns
// four consecutive frames: it reads its planes sixteen bytes at a time (consecutive lanes read consecutive 16-byte pieces: no bank
// conflict), keeps two pieces of each plane in registers and slides through them, so one ds_read_b128 feeds sixteen v_mad_i64_i32.  The taps
// are the same for every lane: they sit in constant memory, reversed and split like the planes, and arrive through scalar loads.  The
// channels' samples meet in an LDS image of the tile's frames and leave as 16-byte stores (ragged tail byte by byte); the peaks are reduced
// per wave, then per block in LDS, then one atomic per block and channel, as in d2d_mix_kernel.
#include <hip/hip_runtime.h>

#include <vector>

#include "../d2d_device.h"
#include "../d2d_launch.h"
#include "d2d_half.h"
#include "d2d_half_internal.h"

namespace d2d {

constexpr int HALF_R = 4;                                        // frames per lane
constexpr int HALF_NCH = ((HALF_NT + 1) / 2 + 3) / 4;            // 16-byte pieces of taps per plane (the odd plane has one tap fewer: zero padded)
constexpr uint32_t HALF_PLANE_PAD = 4u * HALF_NCH + 4u;          // plane entries behind the tile's own: the last lane's window and its look-ahead piece
constexpr uint32_t HALF_MAX_THREADS = 256;
constexpr uint32_t HALF_IMAGE_MAX = 64u * 1024u;                 // bytes of the frame image

struct HalfPlanes { int32_t e[4 * HALF_NCH], o[4 * HALF_NCH]; };
constexpr HalfPlanes half_make_planes() {
    HalfPlanes p{};
    for (int m = 0; m < HALF_NT; ++m) {
        const int32_t q = D2D_HALF_TAPS[HALF_NT - 1 - m];
        if (m & 1) p.o[m >> 1] = q; else p.e[m >> 1] = q;
    }
    return p;
}
__constant__ HalfPlanes half_planes = half_make_planes();

// threads of a block: as many as keep the frame image within HALF_IMAGE_MAX, in whole waves
static uint32_t half_threads(uint32_t frame_bytes) {
    uint32_t t = HALF_IMAGE_MAX / (HALF_R * frame_bytes);
    t = t / 64u * 64u;
    return t < 64u ? 64u : t > HALF_MAX_THREADS ? HALF_MAX_THREADS : t;
}

__global__ __launch_bounds__(HALF_MAX_THREADS) void d2d_half_kernel(const StreamJob* jobs, uint32_t C, int sbits, Epilogue epi) {
    extern __shared__ __align__(16) uint8_t half_lds[];                  // [even plane][odd plane][the frame image]
    __shared__ unsigned long long pkl[HALF_MAX_CHANNELS];                // per channel: the block's peak (non-negative doubles order like their bits)
    const uint32_t sb = epi.sample_bytes, fb = C * sb;
    const uint32_t TILE = HALF_R * blockDim.x, plane = TILE + HALF_PLANE_PAD;
    const StreamJob* fj = jobs + (size_t)blockIdx.y * C;
    const uint32_t nsum = fj[0].nout;
    const uint64_t n0 = fj[0].n0;
    const uint64_t k0 = half_frames_after(n0);
    const uint32_t nk = (uint32_t)(half_frames_after(n0 + nsum) - k0);   // frames of this call (0 for an empty file, and for one odd sum)
    const int32_t r0 = (int32_t)(2 * k0 - n0);                           // the first frame's newest sum, relative to the first new one: 0 or 1
    int32_t* E = reinterpret_cast<int32_t*>(half_lds);
    int32_t* O = E + plane;
    uint8_t* img = half_lds + (size_t)plane * 8u;
    if (threadIdx.x < HALF_MAX_CHANNELS) pkl[threadIdx.x] = 0ull;
    __syncthreads();
    const double ys = ldexp(1.0, -sbits);
    for (uint32_t t0 = blockIdx.x * TILE; t0 < nk; t0 += gridDim.x * TILE) {         // (block-uniform)
        const int32_t base = r0 + 2 * (int32_t)t0 - (int32_t)HALF_HIST;               // s[i] = x[base + i], base >= -HALF_HIST
        for (uint32_t c = 0; c < C; ++c) {
            const StreamJob& job = fj[c];
            const D2D_GLOBAL int32_t* xs = as_global(job.xs);
            for (uint32_t i = threadIdx.x; i < 2u * plane; i += blockDim.x) {
                const int32_t rel = base + (int32_t)i;
                const int32_t v = rel < (int32_t)nsum ? xs[rel] : 0;                  // past the call's sums: read by zero taps and by frames that do not exist
                if (i & 1u) O[i >> 1] = v; else E[i >> 1] = v;
            }
            __syncthreads();
            long long acc[HALF_R];
#pragma unroll
            for (int r = 0; r < HALF_R; ++r) acc[r] = 0;
            const i32x4* Ep = reinterpret_cast<const i32x4*>(E) + threadIdx.x;
            const i32x4* Op = reinterpret_cast<const i32x4*>(O) + threadIdx.x;
            i32x4 ce = Ep[0], co = Op[0];
#pragma unroll 4
            for (int ch = 0; ch < HALF_NCH; ++ch) {
                const i32x4 ne = Ep[ch + 1], no = Op[ch + 1];
                const int32_t we[8] = {ce.x, ce.y, ce.z, ce.w, ne.x, ne.y, ne.z, ne.w};
                const int32_t wo[8] = {co.x, co.y, co.z, co.w, no.x, no.y, no.z, no.w};
#pragma unroll
                for (int a = 0; a < 4; ++a) {
                    const long long qe = half_planes.e[4 * ch + a], qo = half_planes.o[4 * ch + a];
#pragma unroll
                    for (int r = 0; r < HALF_R; ++r) {
                        acc[r] += qe * (long long)we[a + r];
                        acc[r] += qo * (long long)wo[a + r];
                    }
                }
                ce = ne; co = no;
            }
            double pk = 0.0;
#pragma unroll
            for (int r = 0; r < HALF_R; ++r) {
                const uint32_t fr = HALF_R * threadIdx.x + r, t = t0 + fr;
                if (t < nk) pk = fmax(pk, emit_sample(epi, job, half_value(half_round(acc[r]), ys), k0 + t, img + fr * fb + c * sb));
            }
#pragma unroll
            for (int s = 32; s > 0; s >>= 1) pk = fmax(pk, __shfl_xor(pk, s));
            if ((threadIdx.x & 63) == 0 && pk > 0.0) atomicMax(&pkl[c], (unsigned long long)__double_as_longlong(pk));
            __syncthreads();                                                          // the planes are free for the next channel; the last one: the image is whole
        }
        const uint32_t nbytes = min(TILE, nk - t0) * fb;
        uint8_t* out = reinterpret_cast<uint8_t*>(fj[0].out) + (size_t)t0 * fb;       // 16-byte aligned: the buffer is, and a tile's frames are a multiple of 16 bytes
        for (uint32_t i = 16u * threadIdx.x; i < nbytes; i += 16u * blockDim.x) {
            if (i + 16u <= nbytes) *reinterpret_cast<D2D_GLOBAL u32x4*>(as_global(out + i)) = *reinterpret_cast<const u32x4*>(img + i);
            else for (uint32_t k = i; k < nbytes; ++k) out[k] = img[k];
        }
        __syncthreads();
    }
    if (threadIdx.x < C && pkl[threadIdx.x]) atomicMax(reinterpret_cast<unsigned long long*>(fj[threadIdx.x].peak), pkl[threadIdx.x]);
}

// scratch layout per stream: [HALF_HIST carried][nout new]; move the last HALF_HIST to the front (the regions may overlap: every sum is read
// before any is written)
__global__ __launch_bounds__(512) void d2d_half_hist_kernel(const StreamJob* jobs) {
    static_assert(HALF_HIST <= 512, "one thread per carried sum");
    const StreamJob job = jobs[blockIdx.x];
    if (job.nout == 0) return;                                           // (block-uniform)
    int32_t* s = job.xs - HALF_HIST;
    int32_t v = 0;
    if (threadIdx.x < HALF_HIST) v = s[job.nout + threadIdx.x];
    __syncthreads();
    if (threadIdx.x < HALF_HIST) s[threadIdx.x] = v;
}

hipError_t launch_half(const StreamJob* jobs, uint32_t channels, uint32_t nfiles, uint32_t max_sums, int scale_bits, const Epilogue& epi, hipStream_t s) {
    if (nfiles == 0 || max_sums == 0) return hipSuccess;
    if (channels < 1 || channels > HALF_MAX_CHANNELS || epi.channels != channels) return hipErrorInvalidValue;
    const uint32_t threads = half_threads(channels * epi.sample_bytes), tile = HALF_R * threads;
    const uint32_t max_frames = (max_sums + 1u) / 2u;                               // a call of max_sums sums yields at most this many frames
    uint32_t gx = (max_frames + tile - 1u) / tile;
    const uint32_t cap = (8192u + nfiles - 1u) / nfiles;                            // about 8192 blocks in all, each walking its share of the tiles
    if (gx > cap) gx = cap;
    // the planes (2 x (1024 + 196) x 4 = 9.5 KiB at the most) and the frame image (at most HALF_IMAGE_MAX)
    const size_t smem = (size_t)(tile + HALF_PLANE_PAD) * 8u + (size_t)tile * channels * epi.sample_bytes;
    static KernelPrep prep;
    hipError_t e = prep.max_dynamic_lds(reinterpret_cast<const void*>(&d2d_half_kernel), 96 * 1024);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(d2d_half_kernel, dim3(gx, nfiles), dim3(threads), smem, s, jobs, channels, scale_bits, epi);
    return hipGetLastError();
}

hipError_t launch_half_hist(const StreamJob* jobs, uint32_t nstreams, hipStream_t s) {
    if (nstreams == 0) return hipSuccess;
    hipLaunchKernelGGL(d2d_half_hist_kernel, dim3(nstreams), dim3(512), 0, s, jobs);
    return hipGetLastError();
}

}  // namespace d2d

using namespace d2d;

extern "C" int d2d_half_frames_device(d2d_half_job* jobs, uint32_t n_jobs, uint32_t channels, int32_t scale_bits,
                                      uint32_t bit_depth, uint32_t dither, double level_db, uint64_t seed, void* hip_stream) {
    if (int rc = half_check_jobs(jobs, n_jobs, channels, scale_bits, bit_depth, dither, level_db)) return rc;
    const Epilogue epi = mix_epilogue(bit_depth, dither, level_db, seed, channels);
    hipStream_t s = (hipStream_t)hip_stream;
    std::vector<StreamJob> rows((size_t)n_jobs * channels);
    uint32_t max_sums = 0;
    for (uint32_t f = 0; f < n_jobs; ++f) {
        const d2d_half_job& j = jobs[f];
        if (j.frames_out && ((uintptr_t)j.pcm & 15)) return half_fail(D2D_ERR_PARAM, "pcm device pointer must be 16-byte aligned");
        if (j.frames_out && !j.peaks) return half_fail(D2D_ERR_PARAM, "the device form needs a peaks pointer");
        const uint64_t kfirst = half_frames_after(j.first_index);
        for (uint32_t c = 0; c < channels; ++c) {
            StreamJob& r = rows[(size_t)f * channels + c];
            r = StreamJob{};
            r.xs = j.n ? const_cast<int32_t*>(j.sums) + (size_t)c * j.stride + HALF_HIST : nullptr;
            r.out = j.pcm;
            r.peak = j.peaks ? j.peaks + c : nullptr;
            r.n0 = j.first_index; r.nout = (uint32_t)j.n;
            r.ch = r.och = c;
            const uint64_t k = dither_key64(seed, c);
            r.rng_kstep = (uint32_t)k | 1u;
            r.rng_key = (uint32_t)(k >> 32) + (uint32_t)(kfirst >> 32) * r.rng_kstep;
            r.rng_lo0 = (uint32_t)kfirst;
        }
        if (j.n > max_sums) max_sums = (uint32_t)j.n;
    }
    if (rows.empty() || max_sums == 0) return D2D_OK;
    StreamJob* d_rows = nullptr;
    hipError_t he = hipMalloc(reinterpret_cast<void**>(&d_rows), rows.size() * sizeof(StreamJob));
    if (he == hipSuccess) he = hipMemcpyAsync(d_rows, rows.data(), rows.size() * sizeof(StreamJob), hipMemcpyHostToDevice, s);
    if (he == hipSuccess) he = launch_half(d_rows, channels, n_jobs, max_sums, scale_bits, epi, s);
    const hipError_t hs = hipStreamSynchronize(s);
    if (he == hipSuccess) he = hs;
    if (d_rows) (void)hipFree(d_rows);
    if (he != hipSuccess) return half_fail(D2D_ERR_DEVICE, hipGetErrorString(he));
    return D2D_OK;
}
