// d2d_mx_unit.hip -- one object of the fp6 x fp4 FIR kernel: row D2D_MX_UNIT of D2D_MX_UNIT_LIST (d2d_mx.h), so that a clean build spreads over the cores.
#include "d2d_mx_kernel.h"

namespace d2d {
template hipError_t launch_mx_unit<D2D_MX_UNIT>(const FirLaunch& p, uint32_t max_nout, uint32_t nfiles, hipStream_t s);
}  // namespace d2d
