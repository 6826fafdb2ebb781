// mx_scale_probe.hip -- what the scale operands of v_mfma_scale_f32_32x32x64_f8f6f4 do (fp6 e2m3 x fp4 e2m1):
// A = all 1.0, B = all 1.0 -> 64 per element; then with scale bytes e_a / e_b in every byte of the scale registers.
// Then PER-LANE A scales (profiles/rowscale_check.md): a lane's A data is one matrix row, so its scale byte weights that row alone.  Chains of
// twelve MFMAs on random base-32 digits and random stream bits, packed as the fp6 kernel packs them, with the row of digit j scaled by
// 2^0, 2^5, 2^10, 2^15, 2^20 and the digit-4 rows started from -2^28, against the same sums in host integers: every accumulator must hold
// 2^(5j) S_j exactly (profiles/rowscale_check.md records the count).
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdint.h>
#include <stdlib.h>
#include <vector>
typedef int v8i __attribute__((ext_vector_type(8)));
typedef float v16f __attribute__((ext_vector_type(16)));
template <int OA, int OB>
__global__ void k(float* out, int sa, int sb) {
    // e2m3 1.0 = 0b001000; 32 of them = 192 bits: pattern of 6-bit fields 001000 -> bytes repeat every 3: 0x08, 0x82, 0x20
    v8i A = {(int)0x08208208u, (int)0x82082082u, (int)0x20820820u, (int)0x08208208u, (int)0x82082082u, (int)0x20820820u, 0, 0};
    v8i B = {0x22222222, 0x22222222, 0x22222222, 0x22222222, 0, 0, 0, 0};     // e2m1 1.0 = 0b0010
    v16f C = {0};
    C = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(A, B, C, 2, 4, OA, sa, OB, sb);
    if (threadIdx.x == 0) out[0] = C[0];
    if (threadIdx.x == 37) out[1] = C[7];
}

// ---- per-lane A scales ----
constexpr int STEPS = 12, TRIALS = 512, S_BITS = 28;
static int row_digit(int row) { const int rho = 4 * (row >> 3) + (row & 3); return rho < 15 ? rho % 5 : 0; }      // D row -> register 5 q + digit
// one block = one trial: A fragments [STEPS][64 lanes][6 dwords], stream words [STEPS][64 lanes]; out [64 lanes][16]
__global__ void chain_k(const uint32_t* A, const uint32_t* W, const int* sc, float c4, float* out) {
    const uint32_t lane = threadIdx.x, t = blockIdx.x;
    const int scA = sc[lane], scB = (int)0x82828282u;
    v16f acc;
    // the accumulator registers of the digit-4 rows start from c4 (register i of any lane = digit i % 5 below 15)
    for (int i = 0; i < 16; ++i) acc[i] = (i < 15 && i % 5 == 4) ? c4 : 0.0f;
    for (int u = 0; u < STEPS; ++u) {
        const uint32_t* a = A + (((size_t)t * STEPS + u) * 64 + lane) * 6;
        const uint32_t w = W[((size_t)t * STEPS + u) * 64 + lane], w2 = w >> 2;
        const v8i Av = {(int)a[0], (int)a[1], (int)a[2], (int)a[3], (int)a[4], (int)a[5], 0, 0};
        const v8i Bv = {(int)(w & 0x11111111u), (int)(w & 0x22222222u), (int)(w2 & 0x11111111u), (int)(w2 & 0x22222222u), 0, 0, 0, 0};
        acc = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(Av, Bv, acc, 2, 4, 0, scA, 0, scB);
    }
    for (int i = 0; i < 16; ++i) out[((size_t)t * 64 + lane) * 16 + i] = acc[i];
}
static uint32_t e2m3_code(int eighths) {          // the code of eighths / 8 (a multiple of 1/8 up to 2, of 1/4 up to 4)
    const uint32_t s = eighths < 0 ? 32u : 0u;
    const int ax = abs(eighths);
    for (uint32_t c = 0; c < 32; ++c) {
        const uint32_t e = c >> 3, mm = c & 7;
        const int v = e ? (8 + (int)mm) << (e - 1) : (int)mm;
        if (v == ax) return ax == 0 ? 0u : (s | c);
    }
    fprintf(stderr, "%d/8 is not an e2m3 number\n", eighths); exit(2);
}
static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return (uint32_t)(rng_state >> 16); }

// `weights`: exponent of the scale of digit 0..4's rows; returns the number of accumulators that differ from the host integers
static long run_chain(const int (&weights)[5], bool extreme, long* total) {
    std::vector<int8_t> dig((size_t)TRIALS * STEPS * 64 * 32);              // [trial][step][lane][element j]: the digit (lane = row l & 31, K half l >> 5)
    std::vector<uint32_t> A((size_t)TRIALS * STEPS * 64 * 6, 0), W((size_t)TRIALS * STEPS * 64);
    for (size_t i = 0; i < dig.size(); ++i) dig[i] = extreme ? (int8_t)((rnd() & 1) ? 15 : -16) : (int8_t)((int)(rnd() & 31) - 16);
    for (size_t i = 0; i < W.size(); ++i) W[i] = extreme ? 0xFFFFFFFFu : rnd() ^ (rnd() << 16);
    for (size_t f = 0; f < (size_t)TRIALS * STEPS * 64; ++f)
        for (int j = 0; j < 32; ++j) {
            // element j meets B register j >> 3, which arrives as 0.5 (even register) or 1.0 (odd): d/4 or d/8
            const uint32_t code = e2m3_code(((j >> 3) & 1) ? dig[f * 32 + j] : 2 * dig[f * 32 + j]);
            for (int b = 0; b < 6; ++b) if ((code >> b) & 1) A[f * 6 + ((6 * j + b) >> 5)] |= 1u << ((6 * j + b) & 31);
        }
    int sc[64];
    for (int l = 0; l < 64; ++l) sc[l] = (127 + weights[row_digit(l & 31)]) * 0x01010101;
    const float c4 = -ldexpf(1.0f, S_BITS - 20 + weights[4]);
    uint32_t *dA, *dW; int* dS; float* dO;
    hipMalloc(&dA, A.size() * 4); hipMalloc(&dW, W.size() * 4); hipMalloc(&dS, sizeof sc); hipMalloc(&dO, (size_t)TRIALS * 64 * 16 * 4);
    hipMemcpy(dA, A.data(), A.size() * 4, hipMemcpyHostToDevice); hipMemcpy(dW, W.data(), W.size() * 4, hipMemcpyHostToDevice);
    hipMemcpy(dS, sc, sizeof sc, hipMemcpyHostToDevice);
    hipLaunchKernelGGL(chain_k, dim3(TRIALS), dim3(64), 0, 0, dA, dW, dS, c4, dO);
    std::vector<float> O((size_t)TRIALS * 64 * 16);
    if (hipMemcpy(O.data(), dO, O.size() * 4, hipMemcpyDeviceToHost) != hipSuccess) { fprintf(stderr, "the chain kernel failed\n"); exit(3); }
    hipFree(dA); hipFree(dW); hipFree(dS); hipFree(dO);
    long bad = 0, n = 0;
    for (int t = 0; t < TRIALS; ++t)
        for (int l = 0; l < 64; ++l)
            for (int i = 0; i < 15; ++i) {
                // register i of lane l: D row 8 (i / 4) + 4 (l >> 5) + i % 4, column l & 31
                const int row = 8 * (i >> 2) + 4 * (l >> 5) + (i & 3), col = l & 31, dg = row_digit(row);
                int64_t s = dg == 4 ? -((int64_t)1 << (S_BITS - 20)) : 0;
                for (int u = 0; u < STEPS; ++u)
                    for (int kh = 0; kh < 2; ++kh) {
                        const size_t fa = ((size_t)t * STEPS + u) * 64 + (size_t)(32 * kh + row);
                        const uint32_t w = W[((size_t)t * STEPS + u) * 64 + (size_t)(32 * kh + col)];
                        for (int j = 0; j < 32; ++j) if ((w >> (4 * (j & 7) + (j >> 3))) & 1) s += dig[fa * 32 + j];
                    }
                const double want = ldexp((double)s, weights[dg]);
                ++n;
                if ((double)O[((size_t)t * 64 + l) * 16 + i] != want) {
                    if (bad < 5) printf("  trial %d lane %d register %d (digit %d): %.1f, want %.1f\n", t, l, i, dg, O[((size_t)t * 64 + l) * 16 + i], want);
                    ++bad;
                }
            }
    *total = n;
    return bad;
}

int main() {
    float* d; hipMalloc(&d, 64);
    auto run = [&](int ea, int eb) {
        const int sa = ea * 0x01010101, sb = eb * 0x01010101;
        float h[2];
        hipLaunchKernelGGL((k<0, 0>), dim3(1), dim3(64), 0, 0, d, sa, sb); hipMemcpy(h, d, 8, hipMemcpyDeviceToHost);
        printf("scale bytes a=%d b=%d: D = %g, %g (64 = unscaled)\n", ea, eb, h[0], h[1]);
    };
    run(127, 127); run(127, 130); run(130, 127); run(124, 130); run(0, 0);
    // which byte does opsel pick?  bytes 127,128,129,130 from low to high
    float h[2];
    hipLaunchKernelGGL((k<0, 0>), dim3(1), dim3(64), 0, 0, d, 0x7f7f7f7f, (int)0x8281807fu); hipMemcpy(h, d, 8, hipMemcpyDeviceToHost); printf("opsel_b 0: %g\n", h[0]);
    hipLaunchKernelGGL((k<0, 1>), dim3(1), dim3(64), 0, 0, d, 0x7f7f7f7f, (int)0x8281807fu); hipMemcpy(h, d, 8, hipMemcpyDeviceToHost); printf("opsel_b 1: %g\n", h[0]);
    hipLaunchKernelGGL((k<0, 2>), dim3(1), dim3(64), 0, 0, d, 0x7f7f7f7f, (int)0x8281807fu); hipMemcpy(h, d, 8, hipMemcpyDeviceToHost); printf("opsel_b 2: %g\n", h[0]);
    hipLaunchKernelGGL((k<0, 3>), dim3(1), dim3(64), 0, 0, d, 0x7f7f7f7f, (int)0x8281807fu); hipMemcpy(h, d, 8, hipMemcpyDeviceToHost); printf("opsel_b 3: %g\n", h[0]);
    // per-lane A scales: the uniform form first (a control of the probe itself), then both weightings, on random operands and on
    // all-extreme ones (every bit set, every digit 15 or -16)
    const int uniform[5] = {0, 0, 0, 0, 0}, split[5] = {0, 5, 10, 0, 5}, shifted[5] = {0, 5, 10, 15, 20};
    long fails = 0;
    for (int e = 0; e < 2; ++e) {
        long n = 0, b;
        b = run_chain(uniform, e, &n); printf("per-lane A scales, %s operands, uniform 2^0:                %ld mismatches out of %ld\n", e ? "extreme" : "random", b, n); fails += b;
        b = run_chain(split, e, &n);   printf("per-lane A scales, %s operands, 2^0 2^5 2^10 | 2^0 2^5:      %ld mismatches out of %ld\n", e ? "extreme" : "random", b, n); fails += b;
        b = run_chain(shifted, e, &n); printf("per-lane A scales, %s operands, 2^0 2^5 2^10 | 2^15 2^20:    %ld mismatches out of %ld\n", e ? "extreme" : "random", b, n); fails += b;
    }
    return fails ? 1 : 0;
}
