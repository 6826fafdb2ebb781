// d2d_mfma.h -- host view of the int8-MFMA FIR kernels (d2d_kernels_mfma*.hip): launchers and lookups (geometry and tables: d2d_tables.h)
#pragma once
#include <hip/hip_runtime.h>

#include "d2d_tables.h"

namespace d2d {

bool mfma_supported(int M, int N);
size_t mfma_smem_bytes(const MfmaLayout& g, uint32_t channels, uint32_t sample_bytes, uint32_t* waves_per_block);
hipError_t launch_fir_mfma(const FirArgs& a, const MfmaLayout& g, uint32_t max_nout, uint32_t nstreams, hipStream_t s);
const char* mfma_kernel_name(const MfmaLayout& g);
void mfma_debug_stamps(unsigned long long out[8]);   // diagnostic (D2D_DBG=16)

// second-generation kernel (d2d_kernels_mfma2.hip): two phase groups per matrix column
bool mfma2_supported(int M, int N);
size_t mfma2_smem_bytes(int M, int N, uint32_t channels, uint32_t sample_bytes, uint32_t* waves_per_block);
// does this launch shape go to the software-pipelined kernel (d2d_kernels_mfma3.hip)?  Fixed per engine: decides the table variant.
// 0: the two-group kernel itself; 3: the int8 pipelined kernel; 5: the fp6 x fp4 kernel (d2d_kernels_mx.hip)
int mfma2_pipelined(const FirArgs& a, int M, int N);
void mfma2_debug_stamps(unsigned long long out[8]);   // diagnostic (make DIAG=1, D2D_DBG & 256)
hipError_t launch_fir_mfma2(const FirArgs& a, int M, int N, uint32_t max_nout, uint32_t nstreams, hipStream_t s);
void mfma3_debug_stamps(unsigned long long out[8]);  // diagnostic (make DIAG=1, D2D_DBG & 256): per-wave lifetimes of the pipelined kernel

}  // namespace d2d
