// d2d_px_unit.hip -- one object of the direct polyphase kernel: row D2D_PX_UNIT of D2D_PX_UNIT_LIST (d2d_px.h), so that a clean build spreads over the cores.
#include "d2d_px_kernel.h"

namespace d2d {
template hipError_t launch_px_unit<D2D_PX_UNIT>(const FirLaunch& p, uint32_t max_nout, uint32_t nfiles, hipStream_t s);
}  // namespace d2d
