// d2d_m3_unit.hip -- one object of the pipelined int8 FIR kernel: row D2D_M3_UNIT of D2D_M3_UNIT_LIST (d2d_m3.h), so that a clean build spreads over the cores.
#include "d2d_m3_kernel.h"

namespace d2d {
template hipError_t launch_m3_unit<D2D_M3_UNIT>(const FirLaunch& p, uint32_t max_nout, uint32_t nfiles, hipStream_t s);
}  // namespace d2d
