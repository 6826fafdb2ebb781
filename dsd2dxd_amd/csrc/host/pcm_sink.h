// pcm_sink.h -- PCM outputs of the host driver: raw stdout, WAV, AIFF, AIFC, FLAC.
// Counterpart of the reference's writers (`-o S|W|A|C|F`, src/main.rs:98-105,206-214; README.md:6-8).
// The engine hands interleaved little-endian frames (16 / 24-bit container / f32); each sink adapts.
#pragma once
#include <stdint.h>
#include <stdio.h>

#include <string>
#include <vector>

#include "../../../include/dsd2dxd_amd.h"

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
    // A FLAC sink opened with `replaygain`, raw-frame path only: the loudness measured on the GPU (d2d_convert_stream_flac_loud), before
    // close(), which writes it into the REPLAYGAIN_* fields.  Other sinks, and a FLAC sink that saw the samples itself, ignore it.
    // (A sink opened with `true_peak` too expects d2d_loud_true_peak's value in result.peak.)
    virtual void set_loudness(const d2d_loud_result& /*result*/) {}
    // An ALBUM (Rdsd2Pcm::convert_album) keeps its sinks open until every track is measured.  end_stream: no sample follows -- the FLAC
    // sink writes its pending frames and ends its own measurement, so that meter() is complete; "" or error.  meter: the sink's own meter
    // when it measured the samples itself (a FLAC sink opened with `replaygain` on the PCM path), else null.  set_album_loudness: a FLAC
    // sink opened with `album`, before close(), which writes gain_db and peak into the REPLAYGAIN_ALBUM_* fields.  Other sinks ignore all three.
    virtual std::string end_stream() { return ""; }
    virtual const d2d_loud* meter() const { return nullptr; }
    virtual bool meter_has_true_peak_rows() const { return false; }
    virtual void set_album_loudness(const d2d_loud_result& /*album*/) {}
};

// The CPU twin of the loudness measurement behind a stream of write() calls: whole interleaved frames go in as they come, the cells
// of every sub-block they complete go into a meter (d2d_loud_measure_host, d2d_loud_add), and only the pre-roll of the next sub-block
// is kept.  The FLAC sink's host path and `levels --loudness` feed it.  With `true_peak` the same frames also go through the CPU twin
// of the true-peak measurement (d2d_true_peak_measure_host, d2d_loud_add_true_peaks; what holds the pre-roll holds its eleven frames
// of history), and finish() can give d2d_loud_true_peak's value: the `levels --true-peak` and `--replaygain --true-peak` host paths.
class LoudFeed {
   public:
    LoudFeed(uint32_t channels, uint32_t bit_depth, uint32_t rate, bool true_peak = false);
    ~LoudFeed();
    LoudFeed(const LoudFeed&) = delete;
    LoudFeed& operator=(const LoudFeed&) = delete;
    std::string error() const { return err_; }                           // "" or why the meter could not be created
    std::string write(const uint8_t* frames, size_t bytes);              // "" or error
    // the partial last sub-block, then the integration; true_peak (a feed made with `true_peak` only): d2d_loud_true_peak's value, for
    // a stream without a frame the sample peak, 0
    std::string finish(d2d_loud_result* result, double* true_peak = nullptr);
    // the partial last sub-block alone, once (finish() begins with it): afterwards meter() holds the whole stream
    std::string end();
    const d2d_loud* meter() const { return meter_; }
    bool true_peak_rows() const { return tp_rows_; }

   private:
    std::string measure(bool final);
    uint32_t ch_, depth_, rate_;
    size_t fb_;
    d2d_loud* meter_ = nullptr;
    std::vector<uint8_t> pcm_;                                           // the frames from first_ on
    std::vector<d2d_loud_cell> cells_;
    bool tp_ = false, tp_rows_ = false;                                  // true peak asked for; a row of it was added
    bool ended_ = false;                                                 // end() has run
    std::vector<double> peaks_;
    uint64_t first_ = 0, next_ = 0;                                      // pcm_'s first frame; the next sub-block to measure
    std::string err_;
};

// the three fixed-width Vorbis comment values of a result: "-18.00 LUFS", "%+06.2f dB" clamped to +-99.99, "%.6f"
std::string replaygain_reference_text();
std::string replaygain_gain_text(const d2d_loud_result& r);
std::string replaygain_peak_text(const d2d_loud_result& r);

// bit_depth 16/20/24 (integer, 20 in a 24-bit container) or 32 (float).  `id3` = the source's ID3v2
// tag to carry over (may be null or empty): WAV 'id3 ' chunk, AIFF/AIFC 'ID3 ' chunk, FLAC
// VORBIS_COMMENT + PICTURE blocks (id3_tag.h); the raw stdout stream has no place for it.
// `replaygain` (FLAC only; any other type is refused): the file always gets a VORBIS_COMMENT block that ends with
// REPLAYGAIN_REFERENCE_LOUDNESS, REPLAYGAIN_TRACK_GAIN and REPLAYGAIN_TRACK_PEAK -- fields of those names the source had are dropped --
// whose values are placeholders until close() patches them, as it patches STREAMINFO: from the sink's own LoudFeed when it saw the
// samples, from set_loudness on the raw-frame path.  `true_peak` (with `replaygain` only; refused without): REPLAYGAIN_TRACK_PEAK is
// the true peak (d2d_loud_true_peak) instead of the sample peak, in the same fixed-width text, which holds values up to 9.999999 (the
// filter's worst case is 2.03).  `album` (with `replaygain` only; ignored without): REPLAYGAIN_ALBUM_GAIN and REPLAYGAIN_ALBUM_PEAK follow
// the three fields, in the track fields' formats, placeholders until set_album_loudness and close(); the source's REPLAYGAIN_ALBUM_*
// fields are dropped like its track fields.
std::string open_sink(OutputType type, const std::string& path, uint32_t channels, uint32_t rate, uint32_t bit_depth,
                      PcmSink** out, const std::vector<uint8_t>* id3 = nullptr, bool replaygain = false, bool true_peak = false,
                      bool album = false);
const char* output_extension(OutputType t);

}  // namespace d2dhost
