// d2d_launch.h -- host-callable launchers of the device kernels (defined in d2d_kernels*.hip)
#pragma once
#include <hip/hip_runtime.h>

#include <map>
#include <mutex>
#include <string>

#include "../../filters/filter_tables.inc"
#include "d2d_internal.h"

namespace d2d {

// Per-kernel launch preparation.  hipFuncSetAttribute acts on the CURRENT device and engines of one
// process may sit on different GPUs and be driven from different threads (one Rdsd2Pcm per Rayon
// worker, src/main.rs:361-394), so the "already done" state is kept per device under a lock.
struct KernelPrep {
    static constexpr int MAX_DEV = 64;
    std::mutex mu;
    bool attr_done[MAX_DEV] = {};
    // occupancy cache of the persistent MFMA launch
    int blocks_per_cu[MAX_DEV] = {}, ncu[MAX_DEV] = {};
    size_t smem_seen[MAX_DEV] = {};
    uint32_t nwaves_seen[MAX_DEV] = {};
    size_t smem_used[MAX_DEV] = {};          // (the two-group kernel: what its shrink loop settled on)
    uint32_t nwaves_used[MAX_DEV] = {};

    hipError_t max_dynamic_lds(const void* fn, int bytes, int* dev_out = nullptr) {
        int dev = 0;
        hipError_t e = hipGetDevice(&dev);
        if (e != hipSuccess) return e;
        if (dev < 0 || dev >= MAX_DEV) return hipErrorInvalidDevice;
        if (dev_out) *dev_out = dev;
        std::lock_guard<std::mutex> g(mu);
        if (attr_done[dev]) return hipSuccess;
        e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
        if (e == hipSuccess) attr_done[dev] = true;
        return e;
    }
};

// The grid of a persistent launch of the matrix-core FIR kernels: every wave loops over its share of the wave-tiles, so gx = what is resident
// at once (blocks per CU from the occupancy query, cached per device in the kernel's own `prep`, under its lock) spread over the `nrows`
// block rows, and no more than the `need` blocks that have a tile to start on.  (launch_mfma2_t keeps its own copy: it shrinks the block
// inside the query and caches what the register file admitted.)  `nwaves` and `smem` are the plan's: fixed per engine, so the cache holds.
template <class Args>
inline hipError_t persistent_grid_x(void (*kernel)(Args), KernelPrep& prep, int dev, uint32_t nwaves, size_t smem, uint32_t nrows, uint32_t need,
                                    uint32_t* gx_out) {
    int blocks_per_cu, ncu;
    {
        std::lock_guard<std::mutex> g(prep.mu);
        if (prep.blocks_per_cu[dev] == 0 || smem != prep.smem_seen[dev] || nwaves != prep.nwaves_seen[dev]) {
            hipDeviceProp_t prop;
            hipError_t e = hipGetDeviceProperties(&prop, dev);
            if (e != hipSuccess) return e;
            int nb = 0;
            e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, kernel, (int)(64 * nwaves), smem);
            if (e != hipSuccess) return e;
            prep.ncu[dev] = prop.multiProcessorCount;
            prep.blocks_per_cu[dev] = nb < 1 ? 1 : nb;
            prep.smem_seen[dev] = smem; prep.nwaves_seen[dev] = nwaves;
        }
        blocks_per_cu = prep.blocks_per_cu[dev]; ncu = prep.ncu[dev];
    }
    uint32_t gx = (uint32_t)(ncu * blocks_per_cu) / nrows;
    if (gx < 1) gx = 1;
    *gx_out = gx > need ? need : gx;
    return hipSuccess;
}

// The FIR kernel a launcher has just enqueued, spelled the way rocprofv3 prints it: set by every launch_fir_* at the point of the launch
// (per thread: engines are driven from one thread each), copied into the engine by d2d_translate_batch_device, so that
// d2d_kernel_name() reports what ran and not what the dispatch logic predicts.
extern thread_local const char* d2d_last_launched_kernel;
// (one string per (kernel family, instantiation): the family is part of the key -- a function-local static keyed by the int pack alone
// was shared by every family with the same pack, and the first caller's name won)
template <int... V>
inline const char* launched_name(const char* base) {
    static std::mutex mu;
    static std::map<std::string, std::string> names;
    std::lock_guard<std::mutex> g(mu);
    auto it = names.find(base);
    if (it == names.end()) {
        std::string s = std::string(base) + "<";
        const int v[] = {V...};
        for (size_t i = 0; i < sizeof...(V); ++i) s += (i ? ", " : "") + std::to_string(v[i]);
        it = names.emplace(base, s + ">").first;
    }
    return it->second.c_str();       // (map nodes do not move)
}

// The FIR launchers, one per FirFamily.  What they launch was planned when the engine was created (d2d_route.h: FirLaunch); they add what
// depends on the device and the call: the LDS attribute, the occupancy, the grid for `max_nout` outputs of the longest of `nfiles` files.
struct FirLaunch;
typedef hipError_t FirLauncher(const FirLaunch& p, uint32_t max_nout, uint32_t nfiles, hipStream_t s);
FirLauncher launch_fir_lut, launch_fir_mfma, launch_fir_mfma2, launch_fir_mfma3, launch_fir_mx, launch_fir_px, launch_poly_plain;
hipError_t launch_resample2(Rs2Args& a, const d2d_resamp_def& r, uint32_t max_out, uint32_t nfiles, hipStream_t s);
hipError_t launch_deinterleave(const StreamJob* jobs, uint32_t nfiles, uint32_t C, uint32_t streams_per_file, uint32_t max_L, hipStream_t s);
hipError_t launch_noise_shape(const NoiseShapeArgs& a, hipStream_t s);
// tap_bits = 32: frames from the two scratch halves, v = 256 v_hi + v_lo + lo_bias, y = v * 2^-sbits (d2d_kernels.hip)
hipError_t launch_fine_combine(const StreamJob* jobs, uint32_t nstreams, uint32_t max_nout, size_t lo_off, int64_t lo_bias, int sbits,
                               const Epilogue& epi, hipStream_t s);
// a mixed engine's frames from its files' scratch lines: `mix` holds epi.channels x in_channels Q15 coefficients on the device, the lines hold
// y * 2^scale_bits (mix/d2d_mix.hip)
hipError_t launch_mix(const StreamJob* jobs, const int32_t* mix, uint32_t in_channels, uint32_t nfiles, uint32_t max_nout, int scale_bits,
                      const Epilogue& epi, hipStream_t s);
hipError_t launch_history(const StreamJob* jobs, uint32_t nstreams, uint32_t C, uint32_t B, uint32_t keep, hipStream_t s);
// table[c * stride + i] = the dither word of channel c (of `channels`), output n0 + i, i < max_nout, on the keys of the job rows from `job0` on
hipError_t launch_dither_words(const StreamJob* jobs, uint32_t job0, uint32_t channels, uint32_t max_nout, uint32_t* table, uint32_t stride, hipStream_t s);
hipError_t launch_xhist(const StreamJob* jobs, uint32_t nstreams, uint32_t P, hipStream_t s);
// a halved engine's frames from its files' scratch lines (half/d2d_half.hip): job row f * channels + c holds channel c's line (xs: the new
// sums, HALF_HIST carried ones in front), n0 / nout: the first new sum's index and their count, the dither keys of the first FRAME's index;
// the lines hold y * 2^scale_bits.  launch_half_hist then moves every line's last HALF_HIST sums to its front, as launch_xhist does
hipError_t launch_half(const StreamJob* jobs, uint32_t channels, uint32_t nfiles, uint32_t max_sums, int scale_bits, const Epilogue& epi, hipStream_t s);
hipError_t launch_half_hist(const StreamJob* jobs, uint32_t nstreams, hipStream_t s);

}  // namespace d2d
