/* rdsd2pcm_mix_c.h -- the channel-matrix twins of include/rdsd2pcm_c.h: Rdsd2Pcm::set_downmix and ::set_mix behind the file-level C ABI
 * (exported by the same shared library; a header of its own because rdsd2pcm_c.h mirrors the reference crate's surface and nothing else).
 * Call them on a d2dh_conv before d2dh_do_conversion / d2dh_check_level.  0, or D2D_ERR_PARAM with the reason in d2dh_last_error()
 * (the engine's own message for what d2d_create_mix refuses; a container whose layout no preset serves). */
#ifndef RDSD2PCM_MIX_C_H
#define RDSD2PCM_MIX_C_H
#include "rdsd2pcm_c.h"

#ifdef __cplusplus
extern "C" {
#endif

/* target 2: stereo, 1: mono, 0: no mix -- the preset of the container's layout (raw input: by channel count, 4 = quad) */
int d2dh_set_downmix(d2dh_conv* c, uint32_t target);
/* rows x channels Q15 coefficients, row-major (include/dsd2dxd_amd.h: d2d_mix); rows = 0: no mix */
int d2dh_set_mix(d2dh_conv* c, uint32_t rows, const int32_t* coef, size_t count);

#ifdef __cplusplus
}
#endif
#endif
