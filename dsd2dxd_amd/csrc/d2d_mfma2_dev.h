// d2d_mfma2_dev.h -- device-side pieces shared by the two-group matrix-core kernels (d2d_kernels_mfma2.hip and its
// software-pipelined stereo variant d2d_kernels_mfma3.hip): the byte-gather path (launch arguments and staging geometry: d2d_mfma.h).
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "d2d_device.h"
#include "d2d_launch.h"
#include "d2d_mfma.h"

namespace d2d {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

template <int I, int N, class F>
__device__ __forceinline__ void static_for(F&& f) {
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        static_for<I + 1, N>(f);
    }
}

template <int MB>
struct M2Geom {
    static constexpr int RS = 4 * MB;                               // row stride in dwords (16 outputs)
    static constexpr int LSH = m2_lsh(MB);
};

__device__ __forceinline__ void wave_sync2() {
    // LDS operations of one wave execute in order; this only stops the compiler from moving them.
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// 16 bytes of the channel's stream starting at call-relative byte j (any alignment): the slow,
// always-right path (history, ragged blocks, interleaved layouts, call edges)
static __device__ __noinline__ u32x4 gather_chunk(const StreamJob* job, uint32_t C, uint32_t B, uint32_t keep, int32_t j) {
    uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll 1
    for (int b = 0; b < 16; ++b) {
        const uint32_t x = stream_byte(*job, C, B, keep, j + b) << (8 * (b & 3));
        if ((b >> 2) == 0) w[0] |= x; else if ((b >> 2) == 1) w[1] |= x; else if ((b >> 2) == 2) w[2] |= x; else w[3] |= x;
    }
    return u32x4{w[0], w[1], w[2], w[3]};
}

}  // namespace d2d
