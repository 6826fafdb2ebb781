// pcm_sink.h -- PCM outputs of the host driver: raw stdout, WAV, AIFF, AIFC, FLAC.
// Counterpart of the reference's writers (`-o S|W|A|C|F`, src/main.rs:98-105,206-214; README.md:6-8).
// The engine hands interleaved little-endian frames (16 / 24-bit container / f32); each sink adapts.
#pragma once
#include <stdint.h>
#include <stdio.h>

#include <string>
#include <vector>

namespace d2dhost {

enum class OutputType { Stdout, Aiff, Aifc, Wav, Flac };

class PcmSink {
   public:
    virtual ~PcmSink() {}
    virtual std::string write(const uint8_t* frames, size_t bytes) = 0;   // "" or error
    virtual std::string close() = 0;
    // The FLAC sink's raw-frame path (Rdsd2Pcm::set_gpu_flac): frames that d2d_convert_stream_flac encoded on the GPU are written as they
    // come, and STREAMINFO is filled from the stream's stats at close().  Its MD5 field stays 16 zero bytes -- FLAC's "not computed" --
    // because the samples never reach the host, unless set_md5 brings the digest taken on the GPU (Rdsd2Pcm::set_flac_md5).  Every other sink refuses.
    virtual std::string write_frames(const uint8_t*, size_t) { return "this sink takes PCM, not FLAC frames"; }
    virtual void set_frame_stats(uint64_t /*samples_per_channel*/, uint64_t /*blocks*/, uint32_t /*min_frame_bytes*/, uint32_t /*max_frame_bytes*/) {}
    // The FLAC sink's encoder effort (D2D_FLAC_EFFORT_* of include/dsd2dxd_amd.h; 0 unless set), before the first write.  Other sinks ignore it.
    virtual void set_flac_effort(uint32_t /*effort*/) {}
    // The FLAC sink's raw-frame path only: STREAMINFO's MD5 of the samples the frames were made from (d2d_convert_stream_flac_md5), before
    // close().  Other sinks, and a FLAC sink that saw the samples itself, ignore it.
    virtual void set_md5(const uint8_t* /*digest: 16 bytes*/) {}
};

// bit_depth 16/20/24 (integer, 20 in a 24-bit container) or 32 (float).  `id3` = the source's ID3v2
// tag to carry over (may be null or empty): WAV 'id3 ' chunk, AIFF/AIFC 'ID3 ' chunk, FLAC
// VORBIS_COMMENT + PICTURE blocks (id3_tag.h); the raw stdout stream has no place for it.
std::string open_sink(OutputType type, const std::string& path, uint32_t channels, uint32_t rate, uint32_t bit_depth,
                      PcmSink** out, const std::vector<uint8_t>* id3 = nullptr);
const char* output_extension(OutputType t);

}  // namespace d2dhost
