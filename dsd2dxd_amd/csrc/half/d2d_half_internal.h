// d2d_half_internal.h -- what the two halves of the 2:1 decimator's entry points share (half/d2d_half_host.cpp has them): the error slot and
// the checks of a job list.  Not part of the C ABI.
#pragma once
#include <stdint.h>

#include "../../../include/dsd2dxd_amd.h"

namespace d2d {

int half_fail(int code, const char* message);
// every job's bounds and capacity; fills every frames_out once all have passed
int half_check_jobs(d2d_half_job* jobs, uint32_t n_jobs, uint32_t channels, int32_t scale_bits, uint32_t bit_depth, uint32_t dither, double level_db);

}  // namespace d2d
