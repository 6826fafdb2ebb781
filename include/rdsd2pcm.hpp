// rdsd2pcm.hpp -- C++ host-side mirror of the rdsd2pcm crate surface that dsd2dxd's CLI uses
// (/root/reference/src/main.rs:27-31 imports; the crate itself is an absent submodule).  Same names,
// argument order and error texts as the call sites, over the C ABI of dsd2dxd_amd.h; the Rust shim in
// INTEGRATION.md is this file transliterated.
//
//   Rdsd2Pcm::create(...)            <- Rdsd2Pcm::new            (src/main.rs:325-342)
//   Rdsd2Pcm::from_container(...)    <- Rdsd2Pcm::from_container (src/main.rs:362-373)
//   Rdsd2Pcm::new_level_check(...)   <- Rdsd2Pcm::new_level_check (src/bin/dsd_levels/main.rs:214-223)
//   do_conversion(cancel, sender)    <- src/main.rs:345,429       throws std::runtime_error (Err(Box<dyn Error>))
//   check_level(cancel, sender)      <- src/bin/dsd_levels/main.rs:252   returns peak dBFS (f32)
//   file_name()                      <- src/main.rs:398
#pragma once
#include <atomic>
#include <functional>
#include <memory>
#include <optional>
#include <stdexcept>
#include <string>
#include <vector>

namespace rdsd2pcm {

enum class DitherType { TPDF, Rectangular, FPD, None,              // src/main.rs:172-175
                        NoiseShaped };                            // extension ('N'): see dsd2dxd_amd.h
enum class FmtType { Interleaved, Planar };                       // src/main.rs:185-186
enum class Endianness { LsbFirst, MsbFirst };                     // src/main.rs:194-196
enum class FilterType { Equiripple, XLD, Dsd2Pcm, Chebyshev,      // src/main.rs:200-204
                        EquirippleCascade };                      // extension ('S'): the 48 kHz multiples in two stages, see dsd2dxd_amd.h
enum class OutputType { Stdout, Aiff, Aifc, Wav, Flac };          // src/main.rs:208-213

struct ProgressUpdate { float percent; };
constexpr float ONE_HUNDRED_PERCENT = 100.0f;                     // src/main.rs:418
using ProgressSender = std::function<void(const ProgressUpdate&)>;

struct DsdFileFormat {
    enum Kind { Dsf, Dff, Raw, Stdin, Unknown } kind;
    static DsdFileFormat from(const std::string& path);            // src/main.rs:361
    bool is_container() const { return kind == Dsf || kind == Dff; }
};

// src/main.rs:275; throws std::runtime_error
std::vector<std::string> find_dsd_files(const std::vector<std::string>& paths, bool recurse);

class Rdsd2Pcm {
   public:
    // dsd_rate: 1, 2, 4 or 8 (the reference converts it with TryFrom<u32>; an invalid value throws here)
    static Rdsd2Pcm create(size_t bit_depth, OutputType output, double level_db, uint32_t output_rate,
                           std::optional<std::string> out_dir, DitherType dither, FmtType fmt, Endianness endian,
                           uint32_t dsd_rate, uint32_t block_size, size_t channels, FilterType filter,
                           bool append_rate, std::string base_dir, std::optional<std::string> in_path);
    static Rdsd2Pcm from_container(size_t bit_depth, OutputType output, double level_db, uint32_t output_rate,
                                   std::optional<std::string> out_dir, DitherType dither, FilterType filter,
                                   bool append_rate, std::string base_dir, std::string path);
    // path: nullopt = stdin (src/bin/dsd_levels/main.rs:214-223 passes Some(path), :273-281 None)
    // filter: not a reference argument (its level check is always the equiripple filter); EquirippleCascade measures the two-stage definition
    static Rdsd2Pcm new_level_check(uint32_t output_rate, std::optional<std::string> path, FmtType fmt, Endianness endian,
                                    size_t channels, uint32_t block_size, uint32_t input_rate, FilterType filter = FilterType::Equiripple);
    // The three constructors for 44100 and 48000 Hz output (not reference rates; include/dsd2dxd_amd.h, d2d_create_half): the engine converts
    // to twice the rate and halves it with an exact 2:1 decimator behind the FIR.  Same arguments; output_rate is the final rate.  They throw
    // the engine's own message for what d2d_create_half refuses (any other rate, DSD512, DSD256 -> 48000, filters S and D, the noise-shaped
    // dither); set_tap_bits(32) fails when the run starts; set_mix / set_downmix throw.  Sinks, tags, the "-a" suffixes (_44_1K, _48K,
    // " [44.1K]", " [48K]"), ReplayGain, set_true_peak, set_gpu_flac and its switches, convert_album and check_level see an ordinary converter at that rate.
    // create, from_container and new_level_check keep refusing the two rates.
    static Rdsd2Pcm create_half(size_t bit_depth, OutputType output, double level_db, uint32_t output_rate,
                                std::optional<std::string> out_dir, DitherType dither, FmtType fmt, Endianness endian,
                                uint32_t dsd_rate, uint32_t block_size, size_t channels, FilterType filter,
                                bool append_rate, std::string base_dir, std::optional<std::string> in_path);
    static Rdsd2Pcm from_container_half(size_t bit_depth, OutputType output, double level_db, uint32_t output_rate,
                                        std::optional<std::string> out_dir, DitherType dither, FilterType filter,
                                        bool append_rate, std::string base_dir, std::string path);
    static Rdsd2Pcm new_level_check_half(uint32_t output_rate, std::optional<std::string> path, FmtType fmt, Endianness endian,
                                         size_t channels, uint32_t block_size, uint32_t input_rate, FilterType filter = FilterType::Equiripple);
    Rdsd2Pcm(Rdsd2Pcm&&) noexcept;
    Rdsd2Pcm& operator=(Rdsd2Pcm&&) noexcept;
    ~Rdsd2Pcm();

    void do_conversion(const std::atomic<bool>& cancel, ProgressSender sender = nullptr);
    float check_level(const std::atomic<bool>& cancel, ProgressSender sender = nullptr);
    // The tracks of one ALBUM (not a reference call; the C mirror does not have it): FLAC output; every track agrees with the first in
    // every engine parameter and every FLAC switch, else it throws, naming the first track that differs and the field.  With
    // set_gpu_flac all tracks go in lockstep through ONE engine of tracks.size() files (d2d_convert_streams_flac, include/dsd2dxd_amd.h);
    // without it they run one after another on do_conversion's path.  Either way the sinks stay open until the album is measured, and
    // with set_replaygain each file's VORBIS_COMMENT carries REPLAYGAIN_ALBUM_GAIN and REPLAYGAIN_ALBUM_PEAK behind the three track
    // fields (d2d_loud_finish_album over all tracks' 400 ms blocks; the peak is the largest sample peak, with set_true_peak the largest
    // true peak; the source's REPLAYGAIN_ALBUM_* fields are dropped).  Apart from those two fields every file is, byte for byte, what
    // do_conversion writes for its track, and the files of the two paths are equal in every byte.  Progress is the share of the summed
    // bytes; dsp_seconds() and audio_seconds() are the album's on every track afterwards.
    static void convert_album(std::vector<Rdsd2Pcm>& tracks, const std::atomic<bool>& cancel, ProgressSender sender = nullptr);
    std::string file_name() const;
    std::string output_path() const;          // where do_conversion writes ("" for stdout)
    double dsp_seconds() const;               // time inside the engine during the last run (the "DSP speed" figure)
    double audio_seconds() const;
    std::string warnings() const;             // non-fatal findings of the last run (e.g. a damaged ID3 tag that was not copied)
    // engine knobs a driver may set before the run
    void set_device(int device);
    void set_seed(uint64_t seed);
    void set_tap_bits(uint32_t bits);     // 24 (default) or 32: d2d_params.tap_bits (include/dsd2dxd_amd.h); not a reference option
    void set_chunk_bytes(size_t bytes_per_channel);
    // FLAC output only (ignored for every other output type); off by default.  On: the frames are encoded on the GPU
    // (d2d_convert_stream_flac, include/dsd2dxd_amd.h) and only they cross the link.  The file is byte for byte the one the host
    // encoder writes, except STREAMINFO's MD5 field, which is 16 zero bytes -- FLAC's "not computed" -- because the samples never
    // reach the host, unless set_flac_md5 is on.  Tags and pictures are written as before.  Not a reference option; the C mirror (rdsd2pcm_c.h) does not have it.
    void set_gpu_flac(bool on);
    // FLAC output only; 0 by default.  The encoder effort, D2D_FLAC_EFFORT_* of include/dsd2dxd_amd.h: 0 = fixed order 2, one Rice
    // partition, independent channels; 1 = searched fixed predictors, partitioned Rice and stereo modes; 12 = that search with LPC
    // predictors of order 4, 8 and 12.  It applies to the host sink and to the set_gpu_flac path alike, which write the same frames
    // at every effort.  Any other value throws.
    void set_flac_effort(int effort);
    // With set_gpu_flac only (ignored otherwise); off by default.  On: every chunk's frames are parsed, decoded and compared with the PCM
    // they were made from, on the GPU, before they are written (d2d_convert_stream_flac_verified): the counterpart of `flac --verify`.
    // The file is the one written without it; a block that does not verify ends do_conversion with an exception that names the block and
    // the reason.  The C mirror (rdsd2pcm_c.h) does not have it, as it does not have set_gpu_flac.
    void set_flac_verify(bool on);
    // With set_gpu_flac only (ignored otherwise); off by default.  On: the samples are hashed on the GPU as they are made
    // (d2d_convert_stream_flac_md5) and STREAMINFO's MD5 field is filled in: the file is then byte for byte the host encoder's.  It costs
    // one serial MD5 chain per file on the device (README, the FLAC table).  It combines with set_flac_effort and set_flac_verify.  The C
    // mirror (rdsd2pcm_c.h) does not have it, as it does not have set_gpu_flac.
    void set_flac_md5(bool on);
    // FLAC output only (any other output type makes do_conversion throw); off by default.  On: the file's VORBIS_COMMENT block ends with
    // REPLAYGAIN_REFERENCE_LOUDNESS, REPLAYGAIN_TRACK_GAIN and REPLAYGAIN_TRACK_PEAK (BS.1770 integrated loudness against -18 LUFS, the
    // sample peak; include/dsd2dxd_amd.h, "Loudness where the PCM is").  With set_gpu_flac the samples are measured on the GPU
    // (d2d_convert_stream_flac_loud), otherwise by the CPU twin as the sink receives them: the same cells, the same text.  The C mirror
    // (rdsd2pcm_c.h) does not have it, as it does not have the other FLAC switches.
    void set_replaygain(bool on);
    // check_level only; off by default.  On: the float frames of the level check also go through the CPU twin of the loudness
    // measurement; afterwards loudness_valid() says whether any 400 ms block lay above -70 LUFS and loudness_lufs() has the value.
    void set_loudness(bool on);
    bool loudness_valid() const;
    double loudness_lufs() const;
    // off by default.  With set_replaygain: REPLAYGAIN_TRACK_PEAK carries the TRUE peak (the signal oversampled four times;
    // include/dsd2dxd_amd.h, d2d_loud_true_peak) instead of the sample peak, measured on the GPU with set_gpu_flac and by the CPU twin
    // otherwise: the same doubles, the same text.  A conversion with set_true_peak and without set_replaygain throws.  With check_level:
    // the float frames of the level check go through the CPU twin, as with set_loudness, and true_peak_dbtp() has 20 log10 of the
    // value afterwards (-inf for silence).
    void set_true_peak(bool on);
    double true_peak_dbtp() const;
    // Fold the stream's channels down inside the engine, between the FIR sums and the requantiser (d2d_create_mix, include/dsd2dxd_amd.h;
    // not a reference option).  set_downmix(2) / (1): the stereo / mono preset of the container's layout (DSF channel type, DFF CHNL ids; for
    // raw input the channel count decides, 4 channels being quad); a container whose layout no preset serves throws.  set_mix: rows x
    // channels Q15 coefficients, row-major -- swaps, polarity, mid/side.  Either throws the engine's own message for what d2d_create_mix
    // refuses.  0 rows / target 0: no mix.  Sinks, tags, ReplayGain, set_gpu_flac, convert_album and check_level then see
    // output_channels() channels; check_level returns the folded peak.  Without them nothing changes by a byte.
    void set_downmix(uint32_t target);
    void set_mix(uint32_t rows, const std::vector<int32_t>& coef);
    uint32_t output_channels() const;

    struct Impl;                              // opaque state (public only so the .cpp's helpers can name it)

   private:
    std::unique_ptr<Impl> p_;
    explicit Rdsd2Pcm(std::unique_ptr<Impl> p);
    static Rdsd2Pcm make(bool half, size_t bit_depth, OutputType output, double level_db, uint32_t output_rate,
                         std::optional<std::string> out_dir, DitherType dither, FmtType fmt, Endianness endian,
                         uint32_t dsd_rate, uint32_t block_size, size_t channels, FilterType filter,
                         bool append_rate, std::string base_dir, std::optional<std::string> in_path);
    static Rdsd2Pcm make_from_container(bool half, size_t bit_depth, OutputType output, double level_db, uint32_t output_rate,
                                        std::optional<std::string> out_dir, DitherType dither, FilterType filter,
                                        bool append_rate, std::string base_dir, std::string path);
    static Rdsd2Pcm make_level_check(bool half, uint32_t output_rate, std::optional<std::string> path, FmtType fmt, Endianness endian,
                                     size_t channels, uint32_t block_size, uint32_t input_rate, FilterType filter);
};

}  // namespace rdsd2pcm
