// d2d_m3_unit.hip -- one object of the pipelined int8 FIR kernel: row D2D_M3_UNIT of D2D_M3_UNIT_LIST (d2d_m3.h), so that a clean build spreads over the cores.
#include "d2d_m3_kernel.h"

namespace d2d {
template hipError_t launch_m3_unit<D2D_M3_UNIT>(Mfma2Args& m, uint32_t nwt_max, uint32_t nrows, hipStream_t s);
}  // namespace d2d
