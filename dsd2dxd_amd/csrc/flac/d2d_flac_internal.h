// d2d_flac_internal.h -- sizes and the error slot shared by the host and the device side of the FLAC entry points
// (include/dsd2dxd_amd.h, "FLAC frames on the GPU").  Host code only.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <string>

#include "../../../include/dsd2dxd_amd.h"

namespace d2dflac {

constexpr uint32_t BS = D2D_FLAC_BLOCK;
constexpr uint32_t MAX_HEADER_BYTES = 13;      // 4 fixed + 6 frame number + 2 block size + 1 CRC-8

inline bool depth_ok(uint32_t d) { return d == 16 || d == 20 || d == 24; }
inline bool effort_ok(uint32_t e) { return e == D2D_FLAC_EFFORT_FIXED2 || e == D2D_FLAC_EFFORT_SEARCH || e == D2D_FLAC_EFFORT_LPC; }
inline bool verify_method_ok(uint32_t m) { return m == D2D_FLAC_VERIFY_AUTO || m == D2D_FLAC_VERIFY_SERIAL || m == D2D_FLAC_VERIFY_COOP; }
constexpr const char* VERIFY_METHOD_MESSAGE = "unknown FLAC verify method: 0 (auto), 1 (serial) or 2 (cooperative)";
constexpr const char* EFFORT_MESSAGE = "unknown FLAC effort: 0 (fixed order 2), 1 (search) or 12 (search with LPC)";
inline uint32_t sample_bytes(uint32_t depth) { return depth == 16 ? 2 : 3; }
// the header's bound: D2D_FLAC_FRAME_BOUND(n)
inline size_t subframe_bits_bound(uint32_t depth, uint32_t n) { return 19 + 2 * (size_t)depth + 30 * (size_t)(n > 2 ? n - 2 : 0); }
inline size_t frame_bound(uint32_t ch, uint32_t depth, uint32_t n) { return MAX_HEADER_BYTES + 2 + (ch * subframe_bits_bound(depth, n) + 7) / 8; }
inline size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }
inline size_t slot_bytes(uint32_t ch, uint32_t depth) { return align16(frame_bound(ch, depth, BS)); }
constexpr size_t MD5_MAX_FRAMES = (size_t)1 << 56;      // one d2d_flac_md5_update call: frames * frame bytes stays far inside 64 bits
inline size_t block_count(size_t frames, int final) { return frames / BS + ((final && frames % BS) ? 1 : 0); }

// the message d2d_flac_error() returns (thread-local); returns `code`
int fail(int code, const std::string& message);
// "CRC16" for D2D_FLAC_BAD_CRC16, ...
const char* reason_name(uint32_t reason);
#ifdef HIP_INCLUDE_HIP_HIP_RUNTIME_API_H           // (the units that include HIP's host API in front of this header)
// ... with "`what`: HIP's message"; returns D2D_ERR_DEVICE (d2d_flac.hip)
int hip_fail(hipError_t e, const char* what);
#endif

}  // namespace d2dflac
