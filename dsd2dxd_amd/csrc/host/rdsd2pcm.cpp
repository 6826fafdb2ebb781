#include "../../../include/rdsd2pcm.hpp"

#include <math.h>
#include <string.h>
#include <sys/stat.h>

#include <algorithm>
#include <chrono>

#include "../../../include/dsd2dxd_amd.h"
#include "dsd_reader.h"
#include "pcm_sink.h"
#include "id3_tag.h"

namespace rdsd2pcm {

using namespace d2dhost;

DsdFileFormat DsdFileFormat::from(const std::string& path) {
    switch (format_from_path(path)) {
        case d2dhost::DsdFileFormat::Dsf: return {Dsf};
        case d2dhost::DsdFileFormat::Dff: return {Dff};
        case d2dhost::DsdFileFormat::Raw: return {Raw};
        case d2dhost::DsdFileFormat::Stdin: return {Stdin};
        default: return {Unknown};
    }
}

std::vector<std::string> find_dsd_files(const std::vector<std::string>& paths, bool recurse) {
    std::vector<std::string> out;
    std::string err = d2dhost::find_dsd_files(paths, recurse, out);
    if (!err.empty()) throw std::runtime_error(err);
    return out;
}

struct Rdsd2Pcm::Impl {
    d2d_params prm{};
    OutputType output = OutputType::Stdout;
    std::optional<std::string> out_dir;
    bool append_rate = false;
    std::string base_dir;
    std::optional<std::string> in_path;
    DsdInfo info;
    bool level_only = false;
    size_t chunk = 4u << 20;
    bool gpu_flac = false, flac_verify = false, flac_md5 = false, replaygain = false, loudness = false, true_peak = false;
    d2d_loud_result loud_result{};
    double true_peak_value = 0.0;          // d2d_loud_true_peak's value of the last run with true_peak
    uint32_t flac_effort = D2D_FLAC_EFFORT_FIXED2;
    std::string out_path;
    double dsp_s = 0.0, audio_s = 0.0;
    std::string tag_warning;
    int artwork_copied = 0;
    // set_downmix / set_mix: rows x prm.channels Q15 coefficients the engine folds the channels with (d2d_create_mix); empty: no mix
    std::vector<int32_t> mix;
    uint32_t mix_rows = 0;
    // create_half / from_container_half / new_level_check_half: prm.output_rate is 44100 or 48000 and the engine is d2d_create_half's
    bool half = false;
    uint32_t out_channels() const { return mix_rows ? mix_rows : prm.channels; }      // what sinks, tags and meters see
};

// the engine of a run: d2d_create, d2d_create_mix where a mix is set, d2d_create_half for a converter of the halved rates (set_mix keeps a mix away from it)
static int create_engine(const Rdsd2Pcm::Impl& im, uint32_t n_files, d2d_engine** e) {
    if (im.half) return d2d_create_half(&im.prm, n_files, e);
    if (!im.mix_rows) return d2d_create(&im.prm, n_files, e);
    const d2d_mix m{(uint32_t)sizeof(d2d_mix), im.mix_rows, im.mix.data()};
    return d2d_create_mix(&im.prm, &m, n_files, e);
}

static uint32_t dither_code(DitherType d) { return d == DitherType::TPDF ? 'T' : d == DitherType::Rectangular ? 'R' : d == DitherType::FPD ? 'F' : d == DitherType::NoiseShaped ? 'N' : 'X'; }
static uint32_t filter_code(FilterType f) {
    return f == FilterType::Equiripple ? 'E' : f == FilterType::XLD ? 'X' : f == FilterType::Dsd2Pcm ? 'D' : f == FilterType::EquirippleCascade ? 'S' : 'C';
}

static std::string dirname_of(const std::string& p) { size_t s = p.find_last_of('/'); return s == std::string::npos ? "." : (s == 0 ? "/" : p.substr(0, s)); }
static std::string basename_of(const std::string& p) { size_t s = p.find_last_of('/'); return s == std::string::npos ? p : p.substr(s + 1); }
static std::string stem_of(const std::string& p) { std::string b = basename_of(p); size_t d = b.find_last_of('.'); return d == std::string::npos ? b : b.substr(0, d); }

static void mkdirs(const std::string& dir) {
    std::string cur;
    for (size_t i = 0; i <= dir.size(); ++i) {
        if (i == dir.size() || dir[i] == '/') { if (!cur.empty()) mkdir(cur.c_str(), 0777); }
        if (i < dir.size()) cur += dir[i];
    }
}

// "_96K", "_88_2K" (README.md:170-173)
static std::string rate_suffix(uint32_t rate) {
    char b[32];
    if (rate % 1000 == 0) snprintf(b, sizeof(b), "_%uK", rate / 1000);
    else snprintf(b, sizeof(b), "_%u_%uK", rate / 1000, (rate % 1000) / 100);
    return b;
}

static void validate_engine(const d2d_params& p, const bool half) {
    // a dry creation surfaces every parameter error with the engine's own message; a missing GPU is
    // reported later, when the conversion actually starts
    d2d_engine* e = nullptr;
    int rc = half ? d2d_create_half(&p, 1, &e) : d2d_create(&p, 1, &e);
    if (rc == D2D_OK) { d2d_destroy(e); return; }
    if (rc == D2D_ERR_DEVICE) return;
    throw std::runtime_error(d2d_create_error());
}

Rdsd2Pcm::Rdsd2Pcm(std::unique_ptr<Impl> p) : p_(std::move(p)) {}
Rdsd2Pcm::Rdsd2Pcm(Rdsd2Pcm&&) noexcept = default;
Rdsd2Pcm& Rdsd2Pcm::operator=(Rdsd2Pcm&&) noexcept = default;
Rdsd2Pcm::~Rdsd2Pcm() = default;

Rdsd2Pcm Rdsd2Pcm::create(size_t bit_depth, OutputType output, double level_db, uint32_t output_rate,
                          std::optional<std::string> out_dir, DitherType dither, FmtType fmt, Endianness endian,
                          uint32_t dsd_rate, uint32_t block_size, size_t channels, FilterType filter,
                          bool append_rate, std::string base_dir, std::optional<std::string> in_path) {
    return make(false, bit_depth, output, level_db, output_rate, std::move(out_dir), dither, fmt, endian, dsd_rate, block_size, channels, filter, append_rate,
                std::move(base_dir), std::move(in_path));
}
Rdsd2Pcm Rdsd2Pcm::create_half(size_t bit_depth, OutputType output, double level_db, uint32_t output_rate,
                               std::optional<std::string> out_dir, DitherType dither, FmtType fmt, Endianness endian,
                               uint32_t dsd_rate, uint32_t block_size, size_t channels, FilterType filter,
                               bool append_rate, std::string base_dir, std::optional<std::string> in_path) {
    return make(true, bit_depth, output, level_db, output_rate, std::move(out_dir), dither, fmt, endian, dsd_rate, block_size, channels, filter, append_rate,
                std::move(base_dir), std::move(in_path));
}

Rdsd2Pcm Rdsd2Pcm::make(bool half, size_t bit_depth, OutputType output, double level_db, uint32_t output_rate,
                        std::optional<std::string> out_dir, DitherType dither, FmtType fmt, Endianness endian,
                        uint32_t dsd_rate, uint32_t block_size, size_t channels, FilterType filter,
                        bool append_rate, std::string base_dir, std::optional<std::string> in_path) {
    auto im = std::make_unique<Impl>();
    im->half = half;
    d2d_params& p = im->prm;
    p.struct_size = sizeof(p);
    p.dsd_rate = dsd_rate; p.output_rate = output_rate; p.channels = (uint32_t)channels;
    p.fmt = fmt == FmtType::Planar ? D2D_FMT_PLANAR : D2D_FMT_INTERLEAVED;
    p.endianness = endian == Endianness::MsbFirst ? D2D_MSB_FIRST : D2D_LSB_FIRST;
    p.block_size = block_size; p.filter = filter_code(filter); p.bit_depth = (uint32_t)bit_depth;
    p.dither = dither_code(dither); p.kernel = D2D_KERNEL_AUTO; p.device = 0; p.level_db = level_db; p.seed = 0;
    im->output = output; im->out_dir = std::move(out_dir); im->append_rate = append_rate;
    im->base_dir = std::move(base_dir); im->in_path = std::move(in_path);
    im->info.format = im->in_path ? format_from_path(*im->in_path) : d2dhost::DsdFileFormat::Stdin;
    if (im->in_path && im->info.format == d2dhost::DsdFileFormat::Unknown) im->info.format = d2dhost::DsdFileFormat::Raw;
    im->info.channels = p.channels; im->info.dsd_rate = dsd_rate; im->info.planar = p.fmt == D2D_FMT_PLANAR;
    im->info.msb_first = p.endianness == D2D_MSB_FIRST; im->info.block_size = block_size;
    validate_engine(p, half);
    return Rdsd2Pcm(std::move(im));
}

Rdsd2Pcm Rdsd2Pcm::from_container(size_t bit_depth, OutputType output, double level_db, uint32_t output_rate,
                                  std::optional<std::string> out_dir, DitherType dither, FilterType filter,
                                  bool append_rate, std::string base_dir, std::string path) {
    return make_from_container(false, bit_depth, output, level_db, output_rate, std::move(out_dir), dither, filter, append_rate, std::move(base_dir), std::move(path));
}
Rdsd2Pcm Rdsd2Pcm::from_container_half(size_t bit_depth, OutputType output, double level_db, uint32_t output_rate,
                                       std::optional<std::string> out_dir, DitherType dither, FilterType filter,
                                       bool append_rate, std::string base_dir, std::string path) {
    return make_from_container(true, bit_depth, output, level_db, output_rate, std::move(out_dir), dither, filter, append_rate, std::move(base_dir), std::move(path));
}

Rdsd2Pcm Rdsd2Pcm::make_from_container(bool half, size_t bit_depth, OutputType output, double level_db, uint32_t output_rate,
                                       std::optional<std::string> out_dir, DitherType dither, FilterType filter,
                                       bool append_rate, std::string base_dir, std::string path) {
    DsdInfo info;
    std::string err = probe(path, info);
    if (!err.empty()) throw std::runtime_error(err);
    // the container's own layout replaces the command-line flags (README.md:103-105)
    Rdsd2Pcm r = make(half, bit_depth, output, level_db, output_rate, std::move(out_dir), dither,
                        info.planar ? FmtType::Planar : FmtType::Interleaved,
                        info.msb_first ? Endianness::MsbFirst : Endianness::LsbFirst, info.dsd_rate, info.block_size,
                        info.channels, filter, append_rate, std::move(base_dir), path);
    r.p_->info = info;
    return r;
}

Rdsd2Pcm Rdsd2Pcm::new_level_check(uint32_t output_rate, std::optional<std::string> path, FmtType fmt, Endianness endian,
                                   size_t channels, uint32_t block_size, uint32_t input_rate, FilterType filter) {
    return make_level_check(false, output_rate, std::move(path), fmt, endian, channels, block_size, input_rate, filter);
}
Rdsd2Pcm Rdsd2Pcm::new_level_check_half(uint32_t output_rate, std::optional<std::string> path, FmtType fmt, Endianness endian,
                                        size_t channels, uint32_t block_size, uint32_t input_rate, FilterType filter) {
    return make_level_check(true, output_rate, std::move(path), fmt, endian, channels, block_size, input_rate, filter);
}

Rdsd2Pcm Rdsd2Pcm::make_level_check(bool half, uint32_t output_rate, std::optional<std::string> path, FmtType fmt, Endianness endian,
                                    size_t channels, uint32_t block_size, uint32_t input_rate, FilterType filter) {
    Rdsd2Pcm r = (path && DsdFileFormat::from(*path).is_container())
                     ? make_from_container(half, 32, OutputType::Stdout, 0.0, output_rate, std::nullopt, DitherType::None,
                                           filter, false, ".", *path)
                     : make(half, 32, OutputType::Stdout, 0.0, output_rate, std::nullopt, DitherType::None, fmt, endian,
                            input_rate, block_size, channels, filter, false, ".", path);
    r.p_->level_only = true;
    return r;
}

std::string Rdsd2Pcm::file_name() const { return p_->in_path ? basename_of(*p_->in_path) : "stdin"; }
std::string Rdsd2Pcm::output_path() const { return p_->out_path; }
double Rdsd2Pcm::dsp_seconds() const { return p_->dsp_s; }
double Rdsd2Pcm::audio_seconds() const { return p_->audio_s; }
std::string Rdsd2Pcm::warnings() const { return p_->tag_warning; }
void Rdsd2Pcm::set_device(int device) { p_->prm.device = device; }
void Rdsd2Pcm::set_seed(uint64_t seed) { p_->prm.seed = seed; }
void Rdsd2Pcm::set_tap_bits(uint32_t bits) { p_->prm.tap_bits = bits; }
void Rdsd2Pcm::set_chunk_bytes(size_t b) { if (b) p_->chunk = b; }
void Rdsd2Pcm::set_gpu_flac(bool on) { p_->gpu_flac = on; }
void Rdsd2Pcm::set_flac_verify(bool on) { p_->flac_verify = on; }
void Rdsd2Pcm::set_flac_md5(bool on) { p_->flac_md5 = on; }
void Rdsd2Pcm::set_replaygain(bool on) { p_->replaygain = on; }
void Rdsd2Pcm::set_loudness(bool on) { p_->loudness = on; }
bool Rdsd2Pcm::loudness_valid() const { return p_->loud_result.valid != 0; }
double Rdsd2Pcm::loudness_lufs() const { return p_->loud_result.lufs; }
void Rdsd2Pcm::set_true_peak(bool on) { p_->true_peak = on; }
double Rdsd2Pcm::true_peak_dbtp() const { return 20.0 * log10(p_->true_peak_value); }
// The container's layout as a D2D_MIX_LAYOUT_*; for raw input and stdin the channel count decides (4 channels: quad).  0xFFFFFFFF: a
// container whose layout no preset serves.
static uint32_t layout_of(const DsdInfo& info) {
    const uint32_t none = 0xFFFFFFFFu;
    if (info.format == d2dhost::DsdFileFormat::Dsf) {
        static const uint32_t by_type[8] = {none, none, D2D_MIX_LAYOUT_STEREO, D2D_MIX_LAYOUT_LRC, D2D_MIX_LAYOUT_QUAD, D2D_MIX_LAYOUT_LRC_LFE,
                                            D2D_MIX_LAYOUT_5_0, D2D_MIX_LAYOUT_5_1};
        return info.dsf_channel_type < 8 ? by_type[info.dsf_channel_type] : none;
    }
    if (info.format == d2dhost::DsdFileFormat::Dff) {
        std::string ids;
        for (const std::string& id : info.dff_channel_ids) ids += id + "|";
        if (ids == "SLFT|SRGT|") return D2D_MIX_LAYOUT_STEREO;
        if (ids == "SLFT|SRGT|C   |") return D2D_MIX_LAYOUT_LRC;
        if (ids == "SLFT|SRGT|LS  |RS  |") return D2D_MIX_LAYOUT_QUAD;
        if (ids == "SLFT|SRGT|C   |LFE |") return D2D_MIX_LAYOUT_LRC_LFE;
        if (ids == "MLFT|MRGT|C   |LS  |RS  |" || ids == "SLFT|SRGT|C   |LS  |RS  |") return D2D_MIX_LAYOUT_5_0;
        if (ids == "MLFT|MRGT|C   |LFE |LS  |RS  |" || ids == "SLFT|SRGT|C   |LFE |LS  |RS  |") return D2D_MIX_LAYOUT_5_1;
        return none;
    }
    return D2D_MIX_LAYOUT_AUTO;
}

void Rdsd2Pcm::set_downmix(uint32_t target) {
    if (target == 0) { p_->mix.clear(); p_->mix_rows = 0; return; }
    const uint32_t layout = layout_of(p_->info);
    if (layout == 0xFFFFFFFFu) throw std::runtime_error("Invalid downmix: " + file_name() + " states a channel layout no preset serves (use an explicit mix)");
    std::vector<int32_t> coef(2 * (size_t)std::max<uint32_t>(p_->prm.channels, 1));
    uint32_t rows = 0;
    if (d2d_mix_preset(p_->prm.channels, layout, target, coef.data(), &rows) != D2D_OK) throw std::runtime_error(d2d_mix_error());
    coef.resize((size_t)rows * p_->prm.channels);
    set_mix(rows, coef);
}

void Rdsd2Pcm::set_mix(uint32_t rows, const std::vector<int32_t>& coef) {
    if (rows == 0) { p_->mix.clear(); p_->mix_rows = 0; return; }
    if (p_->half) throw std::runtime_error("Invalid mix: 44100 / 48000 output does not combine with a mix");
    if (coef.size() != (size_t)rows * p_->prm.channels) throw std::runtime_error("Invalid mix: it needs rows x channels coefficients, one column per channel of the stream");
    Impl probe = *p_;
    probe.mix = coef; probe.mix_rows = rows;
    // a dry creation, as in validate_engine: the engine's own message for every refusal; a missing GPU is reported when the run starts
    d2d_engine* e = nullptr;
    const int rc = create_engine(probe, 1, &e);
    if (rc == D2D_OK) d2d_destroy(e);
    else if (rc != D2D_ERR_DEVICE) throw std::runtime_error(d2d_create_error());
    p_->mix = coef; p_->mix_rows = rows;
}
uint32_t Rdsd2Pcm::output_channels() const { return p_->out_channels(); }

void Rdsd2Pcm::set_flac_effort(int effort) {
    if (effort != D2D_FLAC_EFFORT_FIXED2 && effort != D2D_FLAC_EFFORT_SEARCH && effort != D2D_FLAC_EFFORT_LPC) throw std::runtime_error("Invalid FLAC effort; must be 0, 1 or 12");
    p_->flac_effort = (uint32_t)effort;
}

namespace {
struct RunCtx {
    DsdSource* src; PcmSink* sink; const std::atomic<bool>* cancel; volatile int cancel_int = 0;
    ProgressSender* sender; std::string io_error;
    LoudFeed* feed = nullptr;              // levels with set_loudness: the frames go here instead of a sink
    std::chrono::steady_clock::duration io_time{};
};
long read_cb(void* u, uint8_t* dst, size_t cap) {
    RunCtx* c = (RunCtx*)u;
    auto t0 = std::chrono::steady_clock::now();
    if (c->cancel->load()) c->cancel_int = 1;
    long n = c->src->read(dst, cap);
    c->io_time += std::chrono::steady_clock::now() - t0;
    return n;
}
int write_cb(void* u, const void* pcm, size_t bytes) {
    RunCtx* c = (RunCtx*)u;
    auto t0 = std::chrono::steady_clock::now();
    std::string e = c->sink ? c->sink->write((const uint8_t*)pcm, bytes) : c->feed ? c->feed->write((const uint8_t*)pcm, bytes) : "";
    c->io_time += std::chrono::steady_clock::now() - t0;
    if (!e.empty()) { c->io_error = e; return 1; }
    if (c->cancel->load()) c->cancel_int = 1;
    return 0;
}
int write_frames_cb(void* u, const void* frames, size_t bytes) {
    RunCtx* c = (RunCtx*)u;
    auto t0 = std::chrono::steady_clock::now();
    std::string e = c->sink->write_frames((const uint8_t*)frames, bytes);
    c->io_time += std::chrono::steady_clock::now() - t0;
    if (!e.empty()) { c->io_error = e; return 1; }
    if (c->cancel->load()) c->cancel_int = 1;
    return 0;
}
void progress_cb(void* u, float pct) {
    RunCtx* c = (RunCtx*)u;
    if (c->sender && *c->sender) (*c->sender)(ProgressUpdate{pct});
}
}  // namespace

// Where a track's output goes and what travels with it: the path below out_dir, the source's tag, the artwork; the sink, opened.
// album: a FLAC sink whose ReplayGain fields include the album's (Rdsd2Pcm::convert_album).
static PcmSink* open_output(Rdsd2Pcm::Impl& im, const DsdInfo& info, bool album) {
    PcmSink* sink = nullptr;
    std::string err;
    if (im.output != OutputType::Stdout) {
        std::string dir;
        const std::string in_dir = im.in_path ? dirname_of(*im.in_path) : ".";
        if (im.out_dir) {
            dir = *im.out_dir;
            // keep the input's position below base_dir (src/main.rs:255-273)
            if (im.in_path && !im.base_dir.empty() && in_dir.compare(0, im.base_dir.size(), im.base_dir) == 0 &&
                in_dir.size() > im.base_dir.size())
                dir += in_dir.substr(im.base_dir.size());
            mkdirs(dir);
        } else dir = in_dir;
        std::string stem = im.in_path ? stem_of(*im.in_path) : "output";
        if (im.append_rate) stem += rate_suffix(im.prm.output_rate);
        im.out_path = dir + "/" + stem + "." + output_extension((d2dhost::OutputType)(int)im.output);
    }
    // the source's ID3v2 tag travels with the audio (README.md:7); -a also marks the album (README.md:170-173)
    std::vector<uint8_t> tag;
    if (im.output != OutputType::Stdout && im.in_path) {
        std::string twarn;
        err = d2dhost::read_source_tag(*im.in_path, info, tag, twarn);
        if (!err.empty()) throw std::runtime_error(err);
        im.tag_warning = twarn;
        if (!tag.empty() && im.append_rate) d2dhost::append_to_album(tag, d2dhost::album_rate_suffix(im.prm.output_rate));
        // -p: artwork next to the sources follows them into the output tree (README.md:115-119)
        if (im.out_dir) im.artwork_copied = d2dhost::copy_artwork(dirname_of(*im.in_path), dirname_of(im.out_path));
    }
    err = open_sink((d2dhost::OutputType)(int)im.output, im.out_path, im.out_channels(), im.prm.output_rate, im.prm.bit_depth, &sink, &tag, im.replaygain, im.true_peak, album);
    if (!err.empty()) throw std::runtime_error(err);
    sink->set_flac_effort(im.flac_effort);
    return sink;
}

static float run(Rdsd2Pcm::Impl& im, const std::atomic<bool>& cancel, ProgressSender& sender, bool levels) {
    DsdSource src;
    std::string err = src.open(im.in_path ? *im.in_path : "-", im.info);
    if (!err.empty()) throw std::runtime_error(err);
    const DsdInfo& info = src.info();
    PcmSink* sink = nullptr;
    im.out_path.clear();
    im.loud_result = d2d_loud_result{};
    im.true_peak_value = 0.0;
    if (!levels && im.true_peak && !im.replaygain)
        throw std::runtime_error("The true peak of a conversion is written as REPLAYGAIN_TRACK_PEAK; it needs set_replaygain (--replaygain)");
    if (!levels && im.replaygain && im.output != OutputType::Flac)
        throw std::runtime_error("ReplayGain tags are written into FLAC files only; choose FLAC output (-o f)");
    if (!levels) sink = open_output(im, info, false);
    std::unique_ptr<PcmSink> sink_guard(sink);
    d2d_engine* e = nullptr;
    if (create_engine(im, 1, &e) != D2D_OK) throw std::runtime_error(d2d_create_error());
    RunCtx ctx; ctx.src = &src; ctx.sink = sink; ctx.cancel = &cancel; ctx.sender = &sender;
    std::unique_ptr<LoudFeed> feed;
    if (levels && (im.loudness || im.true_peak)) {
        feed.reset(new LoudFeed(im.out_channels(), im.prm.bit_depth, im.prm.output_rate, im.true_peak));
        if (!feed->error().empty()) { d2d_destroy(e); throw std::runtime_error(feed->error()); }
        ctx.feed = feed.get();
    }
    auto t0 = std::chrono::steady_clock::now();
    const bool gpu_flac = !levels && im.gpu_flac && im.output == OutputType::Flac && sink;
    int rc;
    std::string msg;
    if (gpu_flac) {
        // the frames are encoded where the PCM is; the sink writes them as they come and takes STREAMINFO's figures from the stats
        size_t chunk = im.chunk;
        const size_t B = im.prm.fmt == D2D_FMT_PLANAR ? im.prm.block_size : 1;
        if (B > 1) chunk = std::max(B, chunk / B * B);                  // whole planar blocks per read, as d2d_convert_stream cuts them
        d2d_flac_stream_stats stats{};
        d2d_flac_check check{};
        uint8_t digest[16];
        d2d_loud* meter = nullptr;
        if (im.replaygain && d2d_loud_create(im.out_channels(), im.prm.output_rate, nullptr, &meter) != D2D_OK) rc = D2D_ERR_PARAM;
        else if (meter && im.true_peak && d2d_loud_set_true_peak(meter, 1) != D2D_OK) { rc = D2D_ERR_PARAM; d2d_loud_destroy(meter); }
        else if (meter) {
            // measured where the PCM is, on the stream that made it
            rc = d2d_convert_stream_flac_loud(e, im.prm.bit_depth, im.flac_effort, read_cb, &ctx, write_frames_cb, &ctx, &ctx.cancel_int,
                                              progress_cb, &ctx, info.bytes_per_channel, chunk, &stats, im.flac_verify ? &check : nullptr,
                                              im.flac_md5 ? digest : nullptr, meter);
            if (!rc) rc = d2d_loud_finish(meter, &im.loud_result);
            if (!rc && im.true_peak) {                                  // (a stream without a frame has no rows: its sample peak, 0)
                im.true_peak_value = im.loud_result.peak;
                if (stats.samples_per_channel) rc = d2d_loud_true_peak(meter, &im.true_peak_value);
                im.loud_result.peak = im.true_peak_value;                // what the sink writes as REPLAYGAIN_TRACK_PEAK
            }
            d2d_loud_destroy(meter);
        } else
        rc = im.flac_md5    ? d2d_convert_stream_flac_md5(e, im.prm.bit_depth, im.flac_effort, read_cb, &ctx, write_frames_cb, &ctx, &ctx.cancel_int,
                                                          progress_cb, &ctx, info.bytes_per_channel, chunk, &stats, im.flac_verify ? &check : nullptr, digest)
           : im.flac_verify ? d2d_convert_stream_flac_verified(e, im.prm.bit_depth, im.flac_effort, read_cb, &ctx, write_frames_cb, &ctx, &ctx.cancel_int,
                                                               progress_cb, &ctx, info.bytes_per_channel, chunk, &stats, &check)
                            : d2d_convert_stream_flac_effort(e, im.prm.bit_depth, im.flac_effort, read_cb, &ctx, write_frames_cb, &ctx, &ctx.cancel_int,
                                                             progress_cb, &ctx, info.bytes_per_channel, chunk, &stats);
        if (rc) msg = d2d_flac_error();
        else {
            sink->set_frame_stats(stats.samples_per_channel, stats.blocks, stats.min_frame_bytes, stats.max_frame_bytes);
            if (im.flac_md5) sink->set_md5(digest);
            if (im.replaygain) sink->set_loudness(im.loud_result);
        }
    } else {
        rc = d2d_convert_stream(e, read_cb, &ctx, levels && !feed ? nullptr : write_cb, &ctx, &ctx.cancel_int,
                                progress_cb, &ctx, info.bytes_per_channel, im.chunk);
        if (rc) msg = d2d_last_error(e);
    }
    auto total = std::chrono::steady_clock::now() - t0;
    float db = 0.f;
    if (!rc && levels) { if (d2d_peak_dbfs(e, 0, &db) != D2D_OK) msg = d2d_last_error(e); }
    if (!rc && feed) { const std::string fe = feed->finish(&im.loud_result, im.true_peak ? &im.true_peak_value : nullptr); if (msg.empty()) msg = fe; }
    const uint64_t bpc = info.bytes_per_channel;
    d2d_destroy(e);
    im.dsp_s = std::chrono::duration<double>(total - ctx.io_time).count();
    im.audio_s = bpc ? (double)bpc * 8.0 / (2822400.0 * im.prm.dsd_rate) : 0.0;
    if (sink) { std::string ce = sink->close(); if (msg.empty() && !ce.empty()) msg = ce; }
    if (!ctx.io_error.empty()) msg = ctx.io_error;
    if (!msg.empty()) throw std::runtime_error(msg);
    return db;
}

void Rdsd2Pcm::do_conversion(const std::atomic<bool>& cancel, ProgressSender sender) { run(*p_, cancel, sender, false); }

float Rdsd2Pcm::check_level(const std::atomic<bool>& cancel, ProgressSender sender) { return run(*p_, cancel, sender, true); }

// ---- an album: all tracks through one engine, the sinks open until the album is measured ----

// the first field in which a track's engine parameters or FLAC switches differ from track 0's; "" when none does
static std::string album_difference(const Rdsd2Pcm::Impl& a, const Rdsd2Pcm::Impl& b) {
    const d2d_params &p = a.prm, &q = b.prm;
#define ALBUM_SAME(field, name) if (!(field)) return name
    ALBUM_SAME(p.dsd_rate == q.dsd_rate, "DSD rate");
    ALBUM_SAME(p.output_rate == q.output_rate, "output rate");
    ALBUM_SAME(p.channels == q.channels, "channel count");
    ALBUM_SAME(p.fmt == q.fmt, "format (planar / interleaved)");
    ALBUM_SAME(p.endianness == q.endianness, "endianness");
    ALBUM_SAME(p.block_size == q.block_size, "block size");
    ALBUM_SAME(p.filter == q.filter, "filter");
    ALBUM_SAME(p.bit_depth == q.bit_depth, "bit depth");
    ALBUM_SAME(p.dither == q.dither, "dither");
    ALBUM_SAME(p.kernel == q.kernel, "kernel");
    ALBUM_SAME(p.device == q.device, "device");
    ALBUM_SAME(p.level_db == q.level_db, "level");
    ALBUM_SAME(p.seed == q.seed, "seed");
    ALBUM_SAME(p.channel_first == q.channel_first && p.channel_count == q.channel_count, "channel subset");
    ALBUM_SAME(p.tap_bits == q.tap_bits, "tap bits");
    ALBUM_SAME(p.debug_flags == q.debug_flags, "debug flags");
    ALBUM_SAME(a.output == b.output, "output type");
    ALBUM_SAME(a.gpu_flac == b.gpu_flac, "GPU FLAC switch");
    ALBUM_SAME(a.flac_effort == b.flac_effort, "FLAC effort");
    ALBUM_SAME(a.flac_verify == b.flac_verify, "FLAC verify switch");
    ALBUM_SAME(a.flac_md5 == b.flac_md5, "FLAC MD5 switch");
    ALBUM_SAME(a.replaygain == b.replaygain, "ReplayGain switch");
    ALBUM_SAME(a.true_peak == b.true_peak, "true-peak switch");
    ALBUM_SAME(a.mix_rows == b.mix_rows && a.mix == b.mix, "mix");
    ALBUM_SAME(a.half == b.half, "halved output rate");
#undef ALBUM_SAME
    return "";
}

// the batch driver polls one cancel flag: every track's callbacks raise it
namespace {
struct AlbumCtx { RunCtx* c; volatile int* cancel; };
long album_read_cb(void* u, uint8_t* dst, size_t cap) {
    AlbumCtx* a = (AlbumCtx*)u;
    const long n = read_cb(a->c, dst, cap);
    if (a->c->cancel_int) *a->cancel = 1;
    return n;
}
int album_write_frames_cb(void* u, const void* frames, size_t bytes) {
    AlbumCtx* a = (AlbumCtx*)u;
    const int rc = write_frames_cb(a->c, frames, bytes);
    if (a->c->cancel_int) *a->cancel = 1;
    return rc;
}
}  // namespace

void Rdsd2Pcm::convert_album(std::vector<Rdsd2Pcm>& tracks, const std::atomic<bool>& cancel, ProgressSender sender) {
    if (tracks.empty()) throw std::runtime_error("An album has at least one track");
    const uint32_t n = (uint32_t)tracks.size();
    Impl& first = *tracks[0].p_;
    for (uint32_t t = 1; t < n; ++t) {
        const std::string d = album_difference(first, *tracks[t].p_);
        if (!d.empty()) throw std::runtime_error("The tracks of an album are converted alike: " + tracks[t].file_name() + " differs from " + tracks[0].file_name() + " in " + d);
    }
    if (first.output != OutputType::Flac) throw std::runtime_error("An album is written as FLAC files; choose FLAC output (-o f)");
    if (first.true_peak && !first.replaygain)
        throw std::runtime_error("The true peak of a conversion is written as REPLAYGAIN_TRACK_PEAK; it needs set_replaygain (--replaygain)");
    const d2d_params& prm = first.prm;
    const bool replaygain = first.replaygain, true_peak = first.true_peak;

    // every track's source and sink, open from here to the end
    std::vector<std::unique_ptr<DsdSource>> srcs(n);
    std::vector<std::unique_ptr<PcmSink>> sinks(n);
    std::vector<RunCtx> ctx(n);
    uint64_t total = 0;
    for (uint32_t t = 0; t < n; ++t) {
        Impl& im = *tracks[t].p_;
        srcs[t].reset(new DsdSource());
        const std::string err = srcs[t]->open(im.in_path ? *im.in_path : "-", im.info);
        if (!err.empty()) throw std::runtime_error(err);
        im.out_path.clear(); im.loud_result = d2d_loud_result{}; im.true_peak_value = 0.0;
        sinks[t].reset(open_output(im, srcs[t]->info(), true));
        ctx[t].src = srcs[t].get(); ctx[t].sink = sinks[t].get(); ctx[t].cancel = &cancel; ctx[t].sender = nullptr;
        total += srcs[t]->info().bytes_per_channel;
    }
    // the GPU path's meters, one per track (the host path's are the sinks' own)
    struct Meters {
        std::vector<d2d_loud*> m;
        ~Meters() { for (d2d_loud* h : m) d2d_loud_destroy(h); }
    } own;
    std::string msg;
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<uint64_t> samples(n, 0);
    if (first.gpu_flac) {
        d2d_engine* e = nullptr;
        if (create_engine(first, n, &e) != D2D_OK) throw std::runtime_error(d2d_create_error());
        size_t chunk = 0;                                               // the batch driver's default, in whole planar blocks (it is a multiple of 4096)
        const size_t B = prm.fmt == D2D_FMT_PLANAR ? prm.block_size : 1;
        if (B > 1 && ((size_t)1 << 19) % B) chunk = std::max(B, ((size_t)1 << 19) / B * B);
        std::vector<d2d_stream_io> io(n);
        std::vector<AlbumCtx> actx(n);
        volatile int album_cancel = 0;
        for (uint32_t t = 0; t < n && msg.empty(); ++t) {
            io[t] = d2d_stream_io{};
            actx[t] = AlbumCtx{&ctx[t], &album_cancel};
            io[t].read = album_read_cb; io[t].read_user = &actx[t]; io[t].write = album_write_frames_cb; io[t].write_user = &actx[t];
            io[t].total_bytes_per_channel = srcs[t]->info().bytes_per_channel;
            if (replaygain) {
                d2d_loud* h = nullptr;
                if (d2d_loud_create(first.out_channels(), prm.output_rate, nullptr, &h) != D2D_OK) { msg = d2d_flac_error(); break; }
                own.m.push_back(h);
                if (true_peak && d2d_loud_set_true_peak(h, 1) != D2D_OK) { msg = d2d_flac_error(); break; }
                io[t].loud = h;
            }
        }
        struct Progress { ProgressSender* s; } pg{&sender};
        d2d_streams_options opt{};
        opt.struct_size = sizeof(opt); opt.bit_depth = prm.bit_depth; opt.effort = first.flac_effort;
        opt.flags = (first.flac_verify ? D2D_STREAMS_VERIFY : 0) | (first.flac_md5 ? D2D_STREAMS_MD5 : 0);
        opt.chunk_bytes_per_channel = chunk; opt.cancel = &album_cancel;
        opt.progress = [](void* u, float pct) { Progress* p = (Progress*)u; if (*p->s && pct < 100.0f) (*p->s)(ProgressUpdate{pct}); };      // (100 is sent once the files are closed)
        opt.progress_user = &pg;
        if (msg.empty() && d2d_convert_streams_flac(e, io.data(), n, &opt) != D2D_OK) msg = d2d_flac_error();
        d2d_destroy(e);
        for (uint32_t t = 0; t < n && msg.empty(); ++t) {
            Impl& im = *tracks[t].p_;
            sinks[t]->set_frame_stats(io[t].stats.samples_per_channel, io[t].stats.blocks, io[t].stats.min_frame_bytes, io[t].stats.max_frame_bytes);
            samples[t] = io[t].stats.samples_per_channel;
            if (first.flac_md5) sinks[t]->set_md5(io[t].md5);
            if (!replaygain) continue;
            if (d2d_loud_finish(own.m[t], &im.loud_result) != D2D_OK) { msg = d2d_flac_error(); break; }
            if (true_peak) {                                            // (a stream without a frame has no rows: its sample peak, 0)
                im.true_peak_value = im.loud_result.peak;
                if (samples[t] && d2d_loud_true_peak(own.m[t], &im.true_peak_value) != D2D_OK) { msg = d2d_flac_error(); break; }
                im.loud_result.peak = im.true_peak_value;
            }
            sinks[t]->set_loudness(im.loud_result);
        }
    } else {
        // one after another on the existing path; progress as the share of the album's bytes
        uint64_t before = 0;
        for (uint32_t t = 0; t < n && msg.empty(); ++t) {
            d2d_engine* e = nullptr;
            if (create_engine(first, 1, &e) != D2D_OK) throw std::runtime_error(d2d_create_error());
            struct Progress { ProgressSender* s; uint64_t before, mine, total; } pg{&sender, before, srcs[t]->info().bytes_per_channel, total};
            auto progress = [](void* u, float pct) {
                Progress* p = (Progress*)u;
                if (!*p->s || !p->total || pct >= 100.0f) return;
                (*p->s)(ProgressUpdate{(float)(100.0 * ((double)p->before + (double)p->mine * pct / 100.0) / (double)p->total)});
            };
            if (d2d_convert_stream(e, read_cb, &ctx[t], write_cb, &ctx[t], &ctx[t].cancel_int, progress, &pg, srcs[t]->info().bytes_per_channel,
                                   tracks[t].p_->chunk) != D2D_OK) msg = d2d_last_error(e);
            d2d_destroy(e);
            if (msg.empty()) msg = sinks[t]->end_stream();
            before += srcs[t]->info().bytes_per_channel;
        }
    }
    for (uint32_t t = 0; t < n; ++t) if (!ctx[t].io_error.empty()) msg = ctx[t].io_error;
    // the album's loudness over every track's meter; its peak the largest sample peak, or the largest true peak
    if (msg.empty() && replaygain) {
        std::vector<const d2d_loud*> meters(n);
        bool rows = true;
        for (uint32_t t = 0; t < n; ++t) {
            meters[t] = first.gpu_flac ? own.m[t] : sinks[t]->meter();
            rows = rows && (first.gpu_flac ? samples[t] != 0 : sinks[t]->meter_has_true_peak_rows());
        }
        d2d_loud_result album{};
        if (d2d_loud_finish_album(meters.data(), n, &album) != D2D_OK) msg = d2d_flac_error();
        else if (true_peak) {
            if (rows) { if (d2d_loud_true_peak_album(meters.data(), n, &album.peak) != D2D_OK) msg = d2d_flac_error(); }
            else                                                        // a track without a frame has no true-peak rows: its sample peak, 0, stands in
                for (uint32_t t = 0; t < n; ++t) {
                    double v = 0.0;
                    if ((first.gpu_flac ? samples[t] != 0 : sinks[t]->meter_has_true_peak_rows()) && d2d_loud_true_peak(meters[t], &v) == D2D_OK && v > album.peak) album.peak = v;
                }
        }
        if (msg.empty()) for (uint32_t t = 0; t < n; ++t) sinks[t]->set_album_loudness(album);
    }
    const auto spent = std::chrono::steady_clock::now() - t0;
    std::chrono::steady_clock::duration io_time{};
    for (uint32_t t = 0; t < n; ++t) io_time += ctx[t].io_time;
    for (uint32_t t = 0; t < n; ++t) {
        const std::string ce = sinks[t]->close();
        if (msg.empty() && !ce.empty()) msg = ce;
    }
    // per album on every track
    double audio = 0.0;
    for (uint32_t t = 0; t < n; ++t) audio += (double)srcs[t]->info().bytes_per_channel * 8.0 / (2822400.0 * prm.dsd_rate);
    for (uint32_t t = 0; t < n; ++t) { tracks[t].p_->dsp_s = std::chrono::duration<double>(spent - io_time).count(); tracks[t].p_->audio_s = audio; }
    if (!msg.empty()) throw std::runtime_error(msg);
    if (sender) sender(ProgressUpdate{ONE_HUNDRED_PERCENT});
}

}  // namespace rdsd2pcm
