// d2d_flac_md5.hip -- STREAMINFO's MD5 on the device (include/dsd2dxd_amd.h, "STREAMINFO's MD5 on the GPU"): d2d_flac_md5_init_device,
// d2d_flac_md5_update_device, d2d_flac_md5_final_device.  The block function, the padding and the 20-bit rule are flac_md5.h, the source
// the host twins (d2d_flac_host.cpp) compile too.
//
// MD5 is serial within a file, so the update kernel gives every file ONE WAVE (a workgroup of 64) and a call's files one launch.  A trip
// of the wave's loop: the 64 lanes fetch up to STAGE bytes of PCM with 16-byte loads into LDS, move them -- through the 20-bit rule where
// it applies -- behind the bytes the state carried (a seam of 0 .. 63 bytes, so the move is byte-granular), and then every lane runs the
// same chain over the whole 64-byte blocks: the message words come back from LDS as broadcasts (one address for the wave), the four
// chaining values are wave-uniform.  What is left behind the last whole block moves to the front for the next trip, and after the last
// into the record.  No workgroup waits for another: no atomics, no spinning, no scratch; every loop is bounded by the frame count the
// host gave.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "d2d_flac_internal.h"
#include "flac_md5.h"

using namespace d2dflac;

namespace {

constexpr uint32_t WAVE = 64;
// S, the PCM bytes of one trip: a multiple of 64 (whole MD5 blocks), of 16 (the loads) and of 3 and 2 (whole samples, so the 20-bit rule
// never sees a sample cut by a trip).  6 loads of 16 bytes per lane.  tests/test_gpu_flac_md5.py places its lengths around S and 2 S.
constexpr uint32_t STAGE = 6144;
constexpr uint32_t MAXF = 128;                                     // files of one launch: 16 bytes of kernel arguments each

static_assert(STAGE % 64 == 0 && STAGE % 16 == 0 && STAGE % 3 == 0, "a trip holds whole blocks, whole loads and whole samples");
static_assert(sizeof(d2d_flac_md5_state) == 96 && offsetof(d2d_flac_md5_state, tail) == 32, "the public layout of the state record");

struct Md5File { const uint8_t* pcm; uint64_t bytes; };
struct Md5Args {
    d2d_flac_md5_state* states;                                    // the record of this launch's file 0
    uint32_t depth20;                                              // non-zero: the 20-bit rule
    uint32_t n_files;
    Md5File f[MAXF];
};
static_assert(sizeof(Md5Args) <= 4096, "the descriptors ride in the kernel arguments");

__global__ __launch_bounds__(WAVE) void flac_md5_update_kernel(const Md5Args a) {
    __shared__ __attribute__((aligned(16))) uint8_t s_raw[STAGE];              // a trip's PCM as it was fetched
    __shared__ __attribute__((aligned(16))) uint8_t s_msg[64 + STAGE];         // the message: the carried tail, then the trip's bytes
    const uint32_t lane = threadIdx.x;
    if (blockIdx.x >= a.n_files) return;
    const Md5File fd = a.f[blockIdx.x];
    if (fd.bytes == 0) return;                                                 // frames == 0: the record stays as it is
    d2d_flac_md5_state* st = a.states + blockIdx.x;
    uint32_t h[4] = {st->h[0], st->h[1], st->h[2], st->h[3]};
    uint32_t t = st->tail_bytes & 63u;                                         // message bytes waiting in front of s_msg
    s_msg[lane] = st->tail[lane];
    const uint32_t* raw32 = reinterpret_cast<const uint32_t*>(s_raw);
    const uint32_t* msg32 = reinterpret_cast<const uint32_t*>(s_msg);

    for (uint64_t off = 0; off < fd.bytes; off += STAGE) {
        const uint32_t n = fd.bytes - off < STAGE ? (uint32_t)(fd.bytes - off) : STAGE;     // this trip's bytes, 1 .. STAGE
        const uint8_t* src = fd.pcm + off;                                     // 16-byte aligned: pcm is, STAGE is a multiple of 16
        // fetch: 16 bytes per lane and load; the last 1 .. 15 bytes of a file singly, so that nothing behind the frames is read
        for (uint32_t c = 16 * lane; c < n; c += 16 * WAVE) {
            if (c + 16 <= n) *reinterpret_cast<uint4*>(s_raw + c) = *reinterpret_cast<const uint4*>(src + c);
            else for (uint32_t k = c; k < n; ++k) s_raw[k] = src[k];
        }
        __syncthreads();
        // behind the seam
        if (a.depth20) {
            for (uint32_t j = 3 * lane; j + 3 <= n; j += 3 * WAVE) {           // a sample per lane (n is a multiple of 3)
                const uint32_t v = d2dmd5::sample20((uint32_t)s_raw[j] | ((uint32_t)s_raw[j + 1] << 8) | ((uint32_t)s_raw[j + 2] << 16));
                s_msg[t + j] = (uint8_t)v; s_msg[t + j + 1] = (uint8_t)(v >> 8); s_msg[t + j + 2] = (uint8_t)(v >> 16);
            }
        } else {
            for (uint32_t j = 4 * lane; j < n; j += 4 * WAVE) {                // a fetched word per lane, its bytes to t + j ..
                const uint32_t v = raw32[j >> 2];
                for (uint32_t k = 0; k < 4; ++k)
                    if (j + k < n) s_msg[t + j + k] = (uint8_t)(v >> (8 * k));
            }
        }
        __syncthreads();
        // the chain, the same in every lane
        const uint32_t avail = t + n, blocks = avail >> 6;                     // avail <= 63 + STAGE: inside s_msg
        for (uint32_t b = 0; b < blocks; ++b) {
            uint32_t m[16];
#pragma unroll
            for (uint32_t i = 0; i < 16; ++i) m[i] = msg32[16 * b + i];
            d2dmd5::block(h, m);
        }
        // what no block took goes to the front
        t = avail & 63u;
        const uint8_t keep = s_msg[(blocks << 6) + lane];                      // (at most 64 * 96 + 63: the buffer's last byte)
        __syncthreads();
        if (lane < t) s_msg[lane] = keep;
        __syncthreads();
    }
    st->tail[lane] = lane < t ? s_msg[lane] : (uint8_t)0;                      // (0 behind the tail: the host twin leaves the same record)
    if (lane == 0) {
        st->h[0] = h[0]; st->h[1] = h[1]; st->h[2] = h[2]; st->h[3] = h[3];
        st->bytes += fd.bytes;
        st->tail_bytes = t;
    }
}

// one lane per file: 96 bytes as six 16-byte stores
__global__ __launch_bounds__(WAVE) void flac_md5_init_kernel(d2d_flac_md5_state* states, uint32_t n_files) {
    const uint32_t f = blockIdx.x * WAVE + threadIdx.x;
    if (f >= n_files) return;
    uint4* p = reinterpret_cast<uint4*>(states + f);
    p[0] = make_uint4(d2dmd5::H0, d2dmd5::H1, d2dmd5::H2, d2dmd5::H3);
    for (int i = 1; i < 6; ++i) p[i] = make_uint4(0, 0, 0, 0);
}

// one lane per file pads a copy of its record and writes the 16 digest bytes
__global__ __launch_bounds__(WAVE) void flac_md5_final_kernel(const d2d_flac_md5_state* states, uint32_t n_files, uint8_t* digests) {
    const uint32_t f = blockIdx.x * WAVE + threadIdx.x;
    if (f >= n_files) return;
    const d2d_flac_md5_state* st = states + f;
    uint8_t digest[16];
    d2dmd5::finish(st->h, st->bytes, st->tail, digest);
#pragma unroll
    for (uint32_t i = 0; i < 16; ++i) digests[(size_t)16 * f + i] = digest[i];
}

int launched(const char* what) {
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? D2D_OK : hip_fail(e, what);
}

}  // namespace

extern "C" int d2d_flac_md5_init_device(void* states, uint32_t n_files, void* hip_stream) {
    if (n_files == 0) return D2D_OK;
    if (!states || ((uintptr_t)states & 15)) return fail(D2D_ERR_PARAM, "states must be a 16-byte aligned pointer the GPU can address");
    hipLaunchKernelGGL(flac_md5_init_kernel, dim3((n_files + WAVE - 1) / WAVE), dim3(WAVE), 0, (hipStream_t)hip_stream,
                       (d2d_flac_md5_state*)states, n_files);
    return launched("flac_md5_init_kernel");
}

extern "C" int d2d_flac_md5_update_device(uint32_t channels, uint32_t bit_depth, const d2d_flac_md5_io* io, uint32_t n_files,
                                          void* states, void* hip_stream) {
    // every check comes before the first device call
    if (!depth_ok(bit_depth)) return fail(D2D_ERR_PARAM, "FLAC holds 16, 20 or 24-bit integers (Invalid bit depth)");
    if (channels == 0 || channels > 8) return fail(D2D_ERR_PARAM, "FLAC holds 1 to 8 channels (Invalid channel count)");
    if (n_files == 0) return D2D_OK;
    if (!io) return fail(D2D_ERR_PARAM, "no files");
    if (!states || ((uintptr_t)states & 15)) return fail(D2D_ERR_PARAM, "states must be a 16-byte aligned pointer the GPU can address");
    for (uint32_t f = 0; f < n_files; ++f) {
        if ((uintptr_t)io[f].pcm & 15) return fail(D2D_ERR_PARAM, "pcm device pointers must be 16-byte aligned");
        if (io[f].frames && !io[f].pcm) return fail(D2D_ERR_PARAM, "pcm device pointers must be non-null");
        if (io[f].frames > MD5_MAX_FRAMES) return fail(D2D_ERR_PARAM, "more frames than a byte count of 64 bits holds");
    }
    const uint64_t fb = (uint64_t)channels * sample_bytes(bit_depth);
    for (uint32_t f0 = 0; f0 < n_files; f0 += MAXF) {
        const uint32_t nf = std::min<uint32_t>(MAXF, n_files - f0);
        Md5Args a{};
        a.states = (d2d_flac_md5_state*)states + f0; a.depth20 = bit_depth == 20; a.n_files = nf;
        bool any = false;
        for (uint32_t i = 0; i < nf; ++i) {
            a.f[i].pcm = (const uint8_t*)io[f0 + i].pcm; a.f[i].bytes = (uint64_t)io[f0 + i].frames * fb;
            any = any || a.f[i].bytes;
        }
        if (!any) continue;
        hipLaunchKernelGGL(flac_md5_update_kernel, dim3(nf), dim3(WAVE), 0, (hipStream_t)hip_stream, a);
        const int rc = launched("flac_md5_update_kernel");
        if (rc != D2D_OK) return rc;
    }
    return D2D_OK;
}

extern "C" int d2d_flac_md5_final_device(const void* states, uint32_t n_files, void* digests, void* hip_stream) {
    if (n_files == 0) return D2D_OK;
    if (!states || ((uintptr_t)states & 15)) return fail(D2D_ERR_PARAM, "states must be a 16-byte aligned pointer the GPU can address");
    if (!digests) return fail(D2D_ERR_PARAM, "null digests pointer");
    hipLaunchKernelGGL(flac_md5_final_kernel, dim3((n_files + WAVE - 1) / WAVE), dim3(WAVE), 0, (hipStream_t)hip_stream,
                       (const d2d_flac_md5_state*)states, n_files, (uint8_t*)digests);
    return launched("flac_md5_final_kernel");
}
