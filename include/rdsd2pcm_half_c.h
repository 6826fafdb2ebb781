/* rdsd2pcm_half_c.h -- the 44.1 / 48 kHz twins of include/rdsd2pcm_c.h's constructors: Rdsd2Pcm::create_half, ::from_container_half and
 * ::new_level_check_half behind the file-level C ABI (exported by the same shared library; a header of its own because rdsd2pcm_c.h
 * mirrors the reference crate's surface and nothing else, and its constructors keep refusing the two rates).
 * Same arguments as d2dh_new / d2dh_from_container / d2dh_new_level_check; output_rate is the final rate, 44100 or 48000.  The converter
 * is then used like any other (d2dh_do_conversion, d2dh_check_level, ...); d2dh_set_mix / d2dh_set_downmix refuse it.
 * 0, or D2D_ERR_PARAM with the reason in d2dh_last_error() (the engine's own message for what d2d_create_half refuses). */
#ifndef RDSD2PCM_HALF_C_H
#define RDSD2PCM_HALF_C_H
#include "rdsd2pcm_c.h"

#ifdef __cplusplus
extern "C" {
#endif

int d2dh_new_half(uint32_t bit_depth, uint32_t output, double level_db, uint32_t output_rate, const char* out_dir, uint32_t dither,
                  uint32_t fmt, uint32_t endian, uint32_t dsd_rate, uint32_t block_size, uint32_t channels, uint32_t filter,
                  int append_rate, const char* base_dir, const char* in_path, d2dh_conv** out);
int d2dh_from_container_half(uint32_t bit_depth, uint32_t output, double level_db, uint32_t output_rate, const char* out_dir,
                             uint32_t dither, uint32_t filter, int append_rate, const char* base_dir, const char* path, d2dh_conv** out);
int d2dh_new_level_check_half(uint32_t output_rate, const char* path, uint32_t fmt, uint32_t endian, uint32_t channels,
                              uint32_t block_size, uint32_t input_rate, d2dh_conv** out);

#ifdef __cplusplus
}
#endif
#endif
