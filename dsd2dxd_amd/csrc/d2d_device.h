// d2d_device.h -- device-side building blocks shared by the FIR kernels:
//   * channel addressing of the packed DSD bytes (planar / interleaved, carried history)
//   * cooperative staging of a channel's byte window into LDS with 16-byte global loads
//   * the epilogue: level, dither, requantise, pack (bit-exact against oracle/d2d_oracle.c)
// Compiled with -ffp-contract=off: every f64 operation is the single IEEE operation written.
#pragma once
#include <hip/hip_runtime.h>

#include "d2d_internal.h"
#include "d2d_sample.h"

namespace d2d {

// Pointers read out of a StreamJob are generic to the compiler; these casts say "global memory"
// so that loads and stores become global_* instead of flat_*.
#define D2D_GLOBAL __attribute__((address_space(1)))
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef int32_t i32x4 __attribute__((ext_vector_type(4)));
template <typename T>
__device__ __forceinline__ D2D_GLOBAL T* as_global(T* p) { return (D2D_GLOBAL T*)(p); }

// a2: byte j of channel `ch` in a call that feeds L bytes per channel.
// planar = [ch0 blk][ch1 blk]..., interleaved = block size 1 (README.md:9 of the reference).
// 32-bit index math: one call feeds fewer than 2^31 bytes per channel.
__device__ __forceinline__ uint64_t layout_addr(uint32_t C, uint32_t B, uint32_t L, uint32_t ch, uint32_t j) {
    if (B == 1) return (uint64_t)j * C + ch;
    const uint32_t blk = (B & (B - 1)) == 0 ? j >> (31 - __builtin_clz(B)) : j / B;
    const uint32_t off = j - blk * B;
    uint32_t blen = L - blk * B;
    if (blen > B) blen = B;
    return (uint64_t)blk * B * C + (uint64_t)ch * blen + off;
}

// One raw byte of the channel's stream at call-relative index j (negative = history).
__device__ __noinline__ uint32_t stream_byte(const StreamJob& job, uint32_t C, uint32_t B, uint32_t keep, int32_t j) {
    if (j < 0) {
        const int32_t h = (int32_t)keep + j;
        return h >= 0 ? as_global(job.hist)[h] : 0u;
    }
    if ((uint32_t)j >= (uint32_t)job.L) return 0u;
    return as_global(job.in)[layout_addr(C, B, (uint32_t)job.L, job.ch, (uint32_t)j)];
}

// Stage the channel bytes [abeg, abeg + nbytes) (abeg % 16 == 0, nbytes % 16 == 0) into LDS.
// Fast path: one global_load_dwordx4 per 16 bytes when the chunk lies inside one planar block
// whose start is 16-byte aligned; otherwise byte gathers (history, short last block, interleaved).
__device__ __forceinline__ void stage_window(uint8_t* lds, const StreamJob& job, uint32_t C, uint32_t B,
                                             uint32_t keep, int64_t abeg64, uint32_t nbytes,
                                             uint32_t tid, uint32_t nthreads) {
    const uint32_t nchunks = nbytes >> 4;
    const bool aligned_layout = (B & 15u) == 0;
    const uint32_t L = (uint32_t)job.L;
    const int32_t abeg = (int32_t)abeg64;
    for (uint32_t q = tid; q < nchunks; q += nthreads) {
        const int32_t j0 = abeg + (int32_t)(q * 16);
        u32x4 v;
        bool fast = false;
        if (aligned_layout && j0 >= 0 && (uint32_t)j0 + 16 <= L) {
            const uint32_t j = (uint32_t)j0;
            const uint32_t blk = (B & (B - 1)) == 0 ? j >> (31 - __builtin_clz(B)) : j / B;
            const uint32_t off = j - blk * B;
            uint32_t blen = L - blk * B;
            if (blen > B) blen = B;
            if ((blen & 15u) == 0) {
                const uint8_t* p = job.in + (uint64_t)blk * B * C + (uint64_t)job.ch * blen + off;
                v = *reinterpret_cast<D2D_GLOBAL const u32x4*>(as_global(p));
                fast = true;
            }
        }
        if (!fast) {
            uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll 1
            for (int b = 0; b < 16; ++b) {
                const uint32_t x = stream_byte(job, C, B, keep, j0 + b) << (8 * (b & 3));
                if ((b >> 2) == 0) w[0] |= x; else if ((b >> 2) == 1) w[1] |= x; else if ((b >> 2) == 2) w[2] |= x; else w[3] |= x;
            }
            v = u32x4{w[0], w[1], w[2], w[3]};
        }
        *reinterpret_cast<u32x4*>(lds + (size_t)q * 16) = v;
    }
}

// the dither word of output index n of the job's channel (d2d_sample.h: dither_word)
__device__ __forceinline__ uint32_t rng32(const StreamJob& job, uint64_t n) {
    return dither_word((uint32_t)n, job.rng_key, job.rng_kstep, job.rng_lo0);
}

// The two steps from x = round(y*scale) (integer depths) or x = round(y*gain) (float) on: dither, then round half away from zero and
// clip, or Airwindows "Dither Float" when dither == 'F' and a plain cast otherwise.  The integer value is returned as it sits in the
// container (20-bit samples already shifted into 24 bits).
__device__ __forceinline__ int32_t finish_int(const Epilogue& ep, double x, uint32_t rnd) {
    double d = 0.0;
    if (ep.dither == 'T') d = dither_f64<DITHER_TRI>(dither_term<DITHER_TRI>(rnd));
    else if (ep.dither == 'R') d = dither_f64<DITHER_RECT>(dither_term<DITHER_RECT>(rnd));
    const int32_t iv = round_clip(x + d, (double)(1u << (ep.bits - 1)));
    return ep.bits == 20 ? iv * 16 : iv;
}
__device__ __forceinline__ float finish_f32(const Epilogue& ep, double x, uint32_t rnd) {
    if (ep.dither == 'F') x = dither_float(x, rnd);
    return (float)x;
}

// a5-a7 from y: level, then the above.  The integer depths keep the operations this was first written with -- the dither
// as a product and a difference (exact, like dither_f64's fma), the clip on the integer (what round_clip does on the f64): the same
// value for every y (tests/test_sample_arithmetic.py), other instructions.
__device__ __forceinline__ int32_t quantise_int(const Epilogue& ep, double y, uint32_t rnd) {
    const double x = y * ep.scale;
    double d = 0.0;
    if (ep.dither == 'T') d = (double)dither_term<DITHER_TRI>(rnd) * 0x1p-16 - 1.0;
    else if (ep.dither == 'R') d = (double)dither_term<DITHER_RECT>(rnd) * 0x1p-17 - 0.5;
    const double q = x + d;
    const double r = trunc(q + copysign(0.5, q));
    const int32_t lim = 1 << (ep.bits - 1);
    int32_t iv = (int32_t)fmax(fmin(r, 2147483520.0), -2147483648.0);
    iv = min(max(iv, -lim), lim - 1);
    return ep.bits == 20 ? iv * 16 : iv;
}
__device__ __forceinline__ float quantise_f32(const Epilogue& ep, double y, uint32_t rnd) { return finish_f32(ep, y * ep.gain, rnd); }

// ---- the variants of the above that need inline asm (matrix-core kernels), device only ----
// round_clip in the integer domain: v_cvt_i32_f64 truncates toward zero and saturates, the clip is one integer med3 (one bound has
// to sit in a VGPR: one SGPR per VOP3 on gfx9).  qmin is uniform.
__device__ __forceinline__ int32_t round_cvt(double q) {
    int32_t ri;
    const double t = q + copysign(0.5, q);
    asm("v_cvt_i32_f64 %0, %1" : "=v"(ri) : "v"(t));
    return ri;
}
__device__ __forceinline__ int32_t round_clip_cvt(double q, int32_t qmin, int32_t qmax_v) {
    int32_t o;
    asm("v_med3_i32 %0, %1, %2, %3" : "=v"(o) : "v"(round_cvt(q)), "s"(qmin), "v"(qmax_v));
    return o;
}
// pk = max(pk, |x|): plain v_max_f64 with the |.| source modifier (fmax() would canonicalise both operands first)
__device__ __forceinline__ void peak_max_abs(double& pk, double x) {
    asm("v_max_f64 %0, %1, |%2|" : "=v"(pk) : "v"(pk), "v"(x));
}
// 24-bit stereo frames k, k+1 (samples La Ra Lb Rb in the low three bytes) -> 12 bytes: [L0 L1 L2 R0 | R1 R2 L0' L1' | L2' R0' R1' R2']
struct S24Pair { uint32_t w0, w1, w2; };
__device__ __forceinline__ S24Pair pack_s24_stereo(uint32_t La, uint32_t Ra, uint32_t Lb, uint32_t Rb) {
    return {__builtin_amdgcn_perm(Ra, La, 0x04020100u), __builtin_amdgcn_perm(Lb, Ra, 0x05040201u), __builtin_amdgcn_perm(Rb, Lb, 0x06050402u)};
}

// One sample straight to memory (used by the LUT and resampler kernels); returns |y*gain|.
__device__ __forceinline__ double emit_sample(const Epilogue& ep, const StreamJob& job, double y, uint64_t n, uint8_t* dst) {
    const uint32_t rnd = rng32(job, n);
    if (ep.bits == 32) {
        *reinterpret_cast<float*>(dst) = quantise_f32(ep, y, rnd);   // frame stride is a multiple of 4 bytes
    } else {
        const int32_t iv = quantise_int(ep, y, rnd);
        if (ep.bits == 16) {
            *reinterpret_cast<uint16_t*>(dst) = (uint16_t)iv;
        } else {
            dst[0] = (uint8_t)iv; dst[1] = (uint8_t)(iv >> 8); dst[2] = (uint8_t)(iv >> 16);
        }
    }
    return fabs(y * ep.gain);
}

// The two samples of a channel PAIR into a wider frame (multichannel files are converted pair by pair): 6 / 4 / 8 bytes that start on an even
// byte of the frame -- one 4-byte and one 2-byte store for 24-bit samples (the three byte stores per sample this replaces were what stage B
// of an 8-channel conversion spent most of its time on), one store otherwise.  The frames' base is 16-byte aligned and the pair's offset
// even, so 2-byte alignment is all these stores have.
typedef uint32_t u32_a2 __attribute__((aligned(2)));
typedef uint32_t u32x2_a2 __attribute__((ext_vector_type(2), aligned(2)));
__device__ __forceinline__ void store_pair_in_frame(uint8_t* dst, uint32_t L, uint32_t R, uint32_t SBY) {
    if (SBY == 3) {
        *reinterpret_cast<D2D_GLOBAL u32_a2*>(as_global(dst)) = (L & 0x00FFFFFFu) | (R << 24);
        *reinterpret_cast<D2D_GLOBAL uint16_t*>(as_global(dst + 4)) = (uint16_t)(R >> 8);
    } else if (SBY == 2) {
        *reinterpret_cast<D2D_GLOBAL u32_a2*>(as_global(dst)) = (L & 0xFFFFu) | (R << 16);
    } else {
        *reinterpret_cast<D2D_GLOBAL u32x2_a2*>(as_global(dst)) = u32x2_a2{L, R};
    }
}

// Which (file, channel group) a block row converts.  The channel groups of one multichannel file write into the SAME frames (a pair's 6 bytes
// of every 24-byte frame of an 8-channel stream), so their partial line writes should meet in one L2: workgroups go to the 8 XCDs round
// robin by their flat index (x fastest), and with one block per row the groups of a file would land on different XCDs, whose L2s cannot
// merge them (stage B of the config-5 shape: 21 ms for 4.4 GB of frames).  Rows y = 8 k ng + 8 s + x (x < 8, s < ng) of whole batches of
// eight files are therefore dealt out as file 8 k + x, group s: the ng blocks of a file sit 8 apart -- same XCD, dispatched together.
// Grids with several blocks per row (gridDim.x a multiple of 8) already have that property and keep the plain order.
__device__ __forceinline__ void row_to_file_group(uint32_t y, uint32_t nrows, uint32_t ng, uint32_t gx, uint32_t& file, uint32_t& grp) {
    const uint32_t batch = 8u * ng;
    if (ng > 1 && (gx & 7u) != 0 && y < nrows / batch * batch) {
        const uint32_t k = y / batch, r = y - k * batch;
        file = 8u * k + (r & 7u); grp = r >> 3;
    } else {
        file = y / ng; grp = y - file * ng;
    }
}

// Non-negative doubles order like their bit patterns: one atomic per block for the peak meter.
__device__ __forceinline__ void block_peak_max(double pk, double* dst, double* lds_red /* [nwaves] */) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) pk = fmax(pk, __shfl_xor(pk, o));
    const uint32_t wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    if ((threadIdx.x & 63) == 0) lds_red[wave] = pk;
    __syncthreads();
    if (threadIdx.x == 0) {
        double m = 0.0;
        for (uint32_t i = 0; i < nw; ++i) m = fmax(m, lds_red[i]);
        if (m > 0.0) atomicMax(reinterpret_cast<unsigned long long*>(dst), (unsigned long long)__double_as_longlong(m));
    }
}

}  // namespace d2d
