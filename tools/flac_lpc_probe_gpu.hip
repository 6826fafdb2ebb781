// flac_lpc_probe_gpu.hip -- tools/flac_lpc_probe.cpp with the routine on the device: d2dlpc::lpc_coefficients of
// dsd2dxd_amd/csrc/flac/flac_lpc.h, as hipcc builds it for gfx950, in a kernel of one thread per workgroup and one workgroup per
// vector -- the way flac_search_kernel runs it, serially in one thread.  tests/test_gpu_flac_search_edges.py compares its lines with the
// g++ probe's and with the Python restatement's.  Built with the flags of csrc/Makefile:
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -o flac_lpc_probe_gpu flac_lpc_probe_gpu.hip
//   ./flac_lpc_probe_gpu R0 R1 ... R12      one vector
//   ./flac_lpc_probe_gpu FILE               many: whitespace-separated integers, thirteen per vector
// prints per vector, in the order given, one line per order 4, 8, 12: "P none" or "P shift q1 ... qP".
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../dsd2dxd_amd/csrc/flac/flac_lpc.h"

using namespace d2dlpc;
constexpr int VEC = MAX_ORDER + 1;

__global__ __launch_bounds__(1) void probe_kernel(const int64_t* R, LpcCoefs* out, uint32_t count) {
    const uint32_t v = blockIdx.x;
    if (v >= count) return;
    int64_t r[VEC];
    for (int l = 0; l < VEC; ++l) r[l] = R[(size_t)v * VEC + l];
    LpcCoefs c = {};
    lpc_coefficients(r, c);
    out[v] = c;
}

#define CHECK(call)                                                                                           \
    do {                                                                                                      \
        const hipError_t e_ = (call);                                                                         \
        if (e_ != hipSuccess) { fprintf(stderr, "flac_lpc_probe_gpu: %s: %s\n", #call, hipGetErrorString(e_)); return 1; } \
    } while (0)

int main(int argc, char** argv) {
    std::vector<int64_t> R;
    if (argc == VEC + 1) {
        for (int l = 0; l < VEC; ++l) R.push_back(strtoll(argv[1 + l], nullptr, 10));
    } else if (argc == 2) {
        FILE* f = fopen(argv[1], "r");
        if (!f) { fprintf(stderr, "flac_lpc_probe_gpu: cannot open %s\n", argv[1]); return 2; }
        long long v;
        while (fscanf(f, "%lld", &v) == 1) R.push_back(v);
        fclose(f);
        if (R.empty() || R.size() % VEC) { fprintf(stderr, "flac_lpc_probe_gpu: %s: not a multiple of thirteen integers\n", argv[1]); return 2; }
    } else {
        fprintf(stderr, "usage: flac_lpc_probe_gpu R0 .. R12 | flac_lpc_probe_gpu FILE\n");
        return 2;
    }
    const uint32_t count = (uint32_t)(R.size() / VEC);
    int64_t* d_R = nullptr;
    LpcCoefs* d_out = nullptr;
    std::vector<LpcCoefs> out(count);
    CHECK(hipMalloc(&d_R, R.size() * sizeof(int64_t)));
    CHECK(hipMalloc(&d_out, count * sizeof(LpcCoefs)));
    CHECK(hipMemcpy(d_R, R.data(), R.size() * sizeof(int64_t), hipMemcpyHostToDevice));
    CHECK(hipMemset(d_out, 0, count * sizeof(LpcCoefs)));
    hipLaunchKernelGGL(probe_kernel, dim3(count), dim3(1), 0, 0, d_R, d_out, count);
    CHECK(hipGetLastError());
    CHECK(hipDeviceSynchronize());
    CHECK(hipMemcpy(out.data(), d_out, count * sizeof(LpcCoefs), hipMemcpyDeviceToHost));
    CHECK(hipFree(d_R));
    CHECK(hipFree(d_out));
    for (uint32_t v = 0; v < count; ++v) {
        const LpcCoefs& c = out[v];
        for (int s = 0; s < CANDIDATES; ++s) {
            const int P = 4 * (s + 1);
            if (!(c.valid >> s & 1u)) { printf("%d none\n", P); continue; }
            printf("%d %d", P, c.shift[s]);
            for (int j = 0; j < P; ++j) printf(" %d", c.q[s][j]);
            printf("\n");
        }
    }
    return 0;
}
