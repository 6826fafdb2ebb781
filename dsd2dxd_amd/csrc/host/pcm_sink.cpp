#include "pcm_sink.h"
#include "md5.h"

#include "id3_tag.h"
#include "../flac/flac_frame_enc.h"

#include <ctype.h>
#include <math.h>

#include <algorithm>
#include <memory>
#include <thread>
#include <string.h>

namespace d2dhost {

const char* output_extension(OutputType t) {
    switch (t) {
        case OutputType::Aiff: return "aif";
        case OutputType::Aifc: return "aifc";
        case OutputType::Wav: return "wav";
        case OutputType::Flac: return "flac";
        default: return "pcm";
    }
}

static void put_le32(uint8_t* p, uint32_t v) { p[0] = v; p[1] = v >> 8; p[2] = v >> 16; p[3] = v >> 24; }
static void put_le16(uint8_t* p, uint16_t v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); }
static void put_be32(uint8_t* p, uint32_t v) { p[3] = v; p[2] = v >> 8; p[1] = v >> 16; p[0] = v >> 24; }
static void put_be16(uint8_t* p, uint16_t v) { p[1] = (uint8_t)v; p[0] = (uint8_t)(v >> 8); }

// ---- loudness on the host: the feed and the tag texts ----

LoudFeed::LoudFeed(uint32_t channels, uint32_t bit_depth, uint32_t rate, bool true_peak)
    : ch_(channels), depth_(bit_depth), rate_(rate), fb_((size_t)channels * (bit_depth == 16 ? 2 : bit_depth == 32 ? 4 : 3)), tp_(true_peak) {
    if (d2d_loud_create(channels, rate, nullptr, &meter_) != D2D_OK) err_ = d2d_flac_error();
    else if (tp_ && d2d_loud_set_true_peak(meter_, 1) != D2D_OK) { err_ = d2d_flac_error(); d2d_loud_destroy(meter_); meter_ = nullptr; }
}
LoudFeed::~LoudFeed() { d2d_loud_destroy(meter_); }

std::string LoudFeed::measure(bool final) {
    const size_t S = rate_ / 10, frames = pcm_.size() / fb_;
    if (!frames) return "";
    cells_.resize((frames / S + 2) * ch_);
    d2d_loud_io io{};
    io.pcm = pcm_.data(); io.frames = frames; io.first_frame = first_; io.first_subblock = next_; io.final = final;
    io.cells = cells_.data(); io.cells_capacity = cells_.size();
    if (d2d_loud_measure_host(ch_, depth_, rate_, &io) != D2D_OK) return d2d_flac_error();
    if (d2d_loud_add(meter_, cells_.data(), io.subblocks, io.cells_out > io.subblocks * ch_) != D2D_OK) return d2d_flac_error();
    if (tp_) {                                                           // the same rows once more
        peaks_.resize(cells_.size());
        d2d_tpeak_io pio{};
        pio.pcm = pcm_.data(); pio.frames = frames; pio.first_frame = first_; pio.first_subblock = next_; pio.final = final;
        pio.peaks = peaks_.data(); pio.peaks_capacity = peaks_.size();
        if (d2d_true_peak_measure_host(ch_, depth_, rate_, &pio) != D2D_OK) return d2d_flac_error();
        if (d2d_loud_add_true_peaks(meter_, peaks_.data(), pio.subblocks, pio.peaks_out > pio.subblocks * ch_) != D2D_OK) return d2d_flac_error();
        if (pio.peaks_out) tp_rows_ = true;
    }
    next_ = io.next_subblock;
    const uint64_t keep_from = (next_ > 2 ? next_ - 2 : 0) * (uint64_t)S;      // the pre-roll of the next sub-block
    pcm_.erase(pcm_.begin(), pcm_.begin() + (size_t)(keep_from - first_) * fb_);
    first_ = keep_from;
    return "";
}

std::string LoudFeed::write(const uint8_t* frames, size_t bytes) {
    if (!meter_) return err_;
    pcm_.insert(pcm_.end(), frames, frames + bytes / fb_ * fb_);
    // (not at every small write: once a sub-block or more is new)
    if ((first_ + pcm_.size() / fb_) / (rate_ / 10) > next_) return measure(false);
    return "";
}

std::string LoudFeed::end() {
    if (!meter_) return err_;
    if (ended_) return "";
    ended_ = true;
    return measure(true);
}

std::string LoudFeed::finish(d2d_loud_result* result, double* true_peak) {
    if (!meter_) return err_;
    const std::string e = end();
    if (!e.empty()) return e;
    if (d2d_loud_finish(meter_, result) != D2D_OK) return d2d_flac_error();
    if (true_peak) {
        if (!tp_) return "this feed does not measure the true peak";
        *true_peak = result->peak;
        if (tp_rows_ && d2d_loud_true_peak(meter_, true_peak) != D2D_OK) return d2d_flac_error();
    }
    return "";
}

std::string replaygain_reference_text() { return "-18.00 LUFS"; }
std::string replaygain_gain_text(const d2d_loud_result& r) {
    char b[32];
    snprintf(b, sizeof(b), "%+06.2f dB", std::max(-99.99, std::min(99.99, r.valid ? r.gain_db : 0.0)));
    return b;
}
std::string replaygain_peak_text(const d2d_loud_result& r) {
    char b[32];
    snprintf(b, sizeof(b), "%.6f", std::max(0.0, std::min(9.999999, r.peak)));
    return b;
}

namespace {

struct RawSink : PcmSink {
    FILE* f;
    explicit RawSink(FILE* fp) : f(fp) {}
    std::string write(const uint8_t* p, size_t n) override { return fwrite(p, 1, n, f) == n ? "" : "short write"; }
    std::string close() override { fflush(f); return ""; }
};

struct WavSink : PcmSink {
    FILE* f; uint32_t ch, rate, bits; uint64_t data = 0; size_t hdr = 0;
    std::vector<uint8_t> id3;
    std::string begin() {
        const uint32_t cont = bits == 16 ? 16 : (bits == 32 ? 32 : 24);
        const bool ext = bits == 20 || ch > 2;                      // valid-bits / channel mask need EXTENSIBLE
        uint8_t h[68]; memset(h, 0, sizeof(h));
        memcpy(h, "RIFF", 4); memcpy(h + 8, "WAVE", 4); memcpy(h + 12, "fmt ", 4);
        const uint32_t fmtsz = ext ? 40 : 16;
        put_le32(h + 16, fmtsz);
        put_le16(h + 20, ext ? 0xFFFE : (bits == 32 ? 3 : 1));
        put_le16(h + 22, (uint16_t)ch); put_le32(h + 24, rate);
        put_le32(h + 28, rate * ch * cont / 8); put_le16(h + 32, (uint16_t)(ch * cont / 8)); put_le16(h + 34, (uint16_t)cont);
        size_t o = 36;
        if (ext) {
            put_le16(h + 36, 22); put_le16(h + 38, (uint16_t)(bits == 32 ? 32 : bits)); put_le32(h + 40, 0);
            static const uint8_t guid_tail[14] = {0x00, 0x00, 0x00, 0x00, 0x10, 0x00, 0x80, 0x00, 0x00, 0xAA, 0x00, 0x38, 0x9B, 0x71};
            put_le16(h + 44, bits == 32 ? 3 : 1); memcpy(h + 46, guid_tail, 14);
            o = 60;
        }
        memcpy(h + o, "data", 4); o += 8;
        hdr = o;
        return fwrite(h, 1, o, f) == o ? "" : "short write";
    }
    std::string write(const uint8_t* p, size_t n) override {
        // RIFF sizes are 32-bit: refuse at the first write that cannot be described, not at close() after hours of output
        if (data + n + hdr + 8 + id3.size() + 2 > 0xFFFFFFFFull) return "WAV output exceeds 4 GiB (RIFF size fields are 32-bit); choose FLAC, a lower rate or depth";
        data += n; return fwrite(p, 1, n, f) == n ? "" : "short write";
    }
    std::string close() override {
        if (data & 1) fputc(0, f);
        uint64_t tail = 0;
        if (!id3.empty()) {                                          // 'id3 ' chunk behind the audio
            uint8_t c[8]; memcpy(c, "id3 ", 4); put_le32(c + 4, (uint32_t)id3.size());
            fwrite(c, 1, 8, f); fwrite(id3.data(), 1, id3.size(), f);
            if (id3.size() & 1) fputc(0, f);
            tail = 8 + id3.size() + (id3.size() & 1);
        }
        if (data + hdr + tail > 0xFFFFFFFFull) { fclose(f); return "WAV output exceeds 4 GiB"; }
        uint8_t v[4];
        put_le32(v, (uint32_t)(hdr - 8 + data + (data & 1) + tail)); fseek(f, 4, SEEK_SET); fwrite(v, 1, 4, f);
        put_le32(v, (uint32_t)data); fseek(f, (long)hdr - 4, SEEK_SET); fwrite(v, 1, 4, f);
        return fclose(f) == 0 ? "" : "close failed";
    }
};

// 80-bit IEEE extended, big-endian (AIFF sample rate)
static void put_ext80(uint8_t* p, double v) {
    memset(p, 0, 10);
    if (v <= 0) return;
    int e; double m = frexp(v, &e);                   // v = m * 2^e, 0.5 <= m < 1
    uint64_t mant = (uint64_t)ldexp(m, 64);
    uint16_t ex = (uint16_t)(e - 1 + 16383);
    put_be16(p, ex);
    for (int i = 0; i < 8; ++i) p[2 + i] = (uint8_t)(mant >> (56 - 8 * i));
}

struct AiffSink : PcmSink {
    FILE* f; uint32_t ch, rate, bits; bool aifc; uint64_t data = 0; size_t comm_frames_at = 0, ssnd_size_at = 0;
    std::vector<uint8_t> tmp, id3;
    std::string begin() {
        const uint32_t cont = bits == 16 ? 16 : (bits == 32 ? 32 : 24);
        std::vector<uint8_t> h;
        auto app = [&](const void* s, size_t n) { h.insert(h.end(), (const uint8_t*)s, (const uint8_t*)s + n); };
        uint8_t b[16];
        app("FORM\0\0\0\0", 8); app(aifc ? "AIFC" : "AIFF", 4);
        if (aifc) { app("FVER", 4); put_be32(b, 4); app(b, 4); put_be32(b, 0xA2805140u); app(b, 4); }
        app("COMM", 4);
        const char* ctype = bits == 32 ? "fl32" : "NONE";
        const char* cname = bits == 32 ? "\x0CIEEE 32-bit\0" : "\x0Enot compressed\0";      // pascal strings, even total
        const size_t cname_len = bits == 32 ? 14 : 16;
        put_be32(b, (uint32_t)(18 + (aifc ? 4 + cname_len : 0))); app(b, 4);
        put_be16(b, (uint16_t)ch); app(b, 2);
        comm_frames_at = h.size(); put_be32(b, 0); app(b, 4);
        put_be16(b, (uint16_t)(bits == 20 ? 20 : cont)); app(b, 2);
        uint8_t e80[10]; put_ext80(e80, (double)rate); app(e80, 10);
        if (aifc) { app(ctype, 4); app(cname, cname_len); }
        app("SSND", 4); ssnd_size_at = h.size(); put_be32(b, 0); app(b, 4); put_be32(b, 0); app(b, 4); put_be32(b, 0); app(b, 4);
        return fwrite(h.data(), 1, h.size(), f) == h.size() ? "" : "short write";
    }
    std::string write(const uint8_t* p, size_t n) override {           // little-endian samples -> big-endian
        const size_t sb = bits == 16 ? 2 : (bits == 32 ? 4 : 3);
        if (data + n + 128 + id3.size() > 0xFFFFFFFFull) return "AIFF output exceeds 4 GiB (FORM size fields are 32-bit); choose FLAC, a lower rate or depth";
        tmp.resize(n);
        for (size_t i = 0; i + sb <= n; i += sb)
            for (size_t k = 0; k < sb; ++k) tmp[i + k] = p[i + sb - 1 - k];
        data += n;
        return fwrite(tmp.data(), 1, n, f) == n ? "" : "short write";
    }
    std::string close() override {
        if (data & 1) fputc(0, f);
        if (!id3.empty()) {                                          // 'ID3 ' chunk behind the audio
            uint8_t c[8]; memcpy(c, "ID3 ", 4); put_be32(c + 4, (uint32_t)id3.size());
            fwrite(c, 1, 8, f); fwrite(id3.data(), 1, id3.size(), f);
            if (id3.size() & 1) fputc(0, f);
        }
        const size_t sb = bits == 16 ? 2 : (bits == 32 ? 4 : 3);
        long end = ftell(f);
        if ((uint64_t)end > 0xFFFFFFFFull) { fclose(f); return "AIFF output exceeds 4 GiB"; }
        uint8_t v[4];
        put_be32(v, (uint32_t)(end - 8)); fseek(f, 4, SEEK_SET); fwrite(v, 1, 4, f);
        put_be32(v, (uint32_t)(data / (sb * ch))); fseek(f, (long)comm_frames_at, SEEK_SET); fwrite(v, 1, 4, f);
        put_be32(v, (uint32_t)(data + 8)); fseek(f, (long)ssnd_size_at, SEEK_SET); fwrite(v, 1, 4, f);
        return fclose(f) == 0 ? "" : "close failed";
    }
};

// Md5, of the unencoded audio for STREAMINFO, lives in md5.h: the CLI's `verify` hashes the decoded samples with the same code.

// FlacFrameEnc, the frame encoder, lives in ../flac/flac_frame_enc.h: d2d_flac_encode_host runs the same code.

struct FlacSink : PcmSink {
    FILE* f; uint32_t ch, rate, bits; uint64_t frames = 0; uint32_t frame_no = 0;
    static constexpr uint32_t BS = 4096;
    std::vector<int32_t> buf;      // interleaved pending samples
    uint32_t min_fs = 0xFFFFFF, max_fs = 0;
    std::vector<uint8_t> id3;
    Md5 md5;                       // of the samples as little-endian whole-byte integers, interleaved (FLAC format, STREAMINFO)
    std::vector<FlacFrameEnc> encs;
    bool io_failed = false;
    bool raw_frames = false;       // the frames came encoded (write_frames): no samples were seen, so there is no MD5 unless set_md5 brings one
    bool have_digest = false; uint8_t digest[16];
    void set_md5(const uint8_t* d) override { memcpy(digest, d, 16); have_digest = true; }
    uint32_t effort = 0;           // flac_frame_enc.h: 0 = fixed order 2, 1 = the search, 12 = the search with LPC
    void set_flac_effort(uint32_t e) override { effort = e; }
    // ReplayGain (open_sink's `replaygain`): where the two values lie in the file, the sink's own meter, the GPU path's result
    bool replaygain = false, true_peak = false, album = false;
    long gain_at = 0, peak_at = 0, album_gain_at = 0, album_peak_at = 0;
    bool have_album = false; d2d_loud_result album_loudness{};
    void set_album_loudness(const d2d_loud_result& r) override { album_loudness = r; have_album = true; }
    std::string end_stream() override {
        drain(true);
        if (io_failed) return "short write";
        return feed && !raw_frames ? feed->end() : "";
    }
    const d2d_loud* meter() const override { return feed && !raw_frames ? feed->meter() : nullptr; }
    bool meter_has_true_peak_rows() const override { return feed && !raw_frames && feed->true_peak_rows(); }
    std::unique_ptr<LoudFeed> feed;
    bool have_loudness = false; d2d_loud_result loudness{};
    void set_loudness(const d2d_loud_result& r) override { loudness = r; have_loudness = true; }
    uint32_t depth() const { return bits == 20 ? 20 : bits; }
    std::string begin() {
        // metadata: STREAMINFO (filled in at close), then the source's tag as VORBIS_COMMENT and PICTURE
        // blocks; the last block carries the 0x80 flag
        std::vector<std::pair<std::string, std::string>> fields;
        std::vector<TagPicture> pics;
        tag_to_vorbis(id3, fields, pics);
        size_t gain_in_block = 0, peak_in_block = 0, album_gain_in_block = 0, album_peak_in_block = 0;
        if (replaygain) {
            // the source's own loudness fields go, ours come last: placeholders of the final width, patched at close()
            auto ours = [this](std::string k) {
                for (char& c : k) c = (char)toupper((unsigned char)c);
                return k.rfind("REPLAYGAIN_TRACK_", 0) == 0 || k == "REPLAYGAIN_REFERENCE_LOUDNESS" || (album && k.rfind("REPLAYGAIN_ALBUM_", 0) == 0);
            };
            fields.erase(std::remove_if(fields.begin(), fields.end(), [&](const std::pair<std::string, std::string>& kv) { return ours(kv.first); }), fields.end());
            const d2d_loud_result none{};
            fields.push_back({"REPLAYGAIN_REFERENCE_LOUDNESS", replaygain_reference_text()});
            fields.push_back({"REPLAYGAIN_TRACK_GAIN", replaygain_gain_text(none)});
            fields.push_back({"REPLAYGAIN_TRACK_PEAK", replaygain_peak_text(none)});
            if (album) {
                fields.push_back({"REPLAYGAIN_ALBUM_GAIN", replaygain_gain_text(none)});
                fields.push_back({"REPLAYGAIN_ALBUM_PEAK", replaygain_peak_text(none)});
            }
            feed.reset(new LoudFeed(ch, bits, rate, true_peak));
            if (!feed->error().empty()) return feed->error();
        }
        std::vector<std::vector<uint8_t>> blocks;
        if (!fields.empty()) {
            std::vector<uint8_t> b;
            auto le32 = [&](uint32_t v) { uint8_t t[4]; put_le32(t, v); b.insert(b.end(), t, t + 4); };
            const std::string vendor = "dsd2dxd_amd";
            le32((uint32_t)vendor.size()); b.insert(b.end(), vendor.begin(), vendor.end());
            le32((uint32_t)fields.size());
            for (const auto& kv : fields) {
                const std::string e = kv.first + "=" + kv.second;
                le32((uint32_t)e.size());
                if (replaygain && kv.first == "REPLAYGAIN_TRACK_GAIN") gain_in_block = b.size() + kv.first.size() + 1;
                if (replaygain && kv.first == "REPLAYGAIN_TRACK_PEAK") peak_in_block = b.size() + kv.first.size() + 1;
                if (replaygain && album && kv.first == "REPLAYGAIN_ALBUM_GAIN") album_gain_in_block = b.size() + kv.first.size() + 1;
                if (replaygain && album && kv.first == "REPLAYGAIN_ALBUM_PEAK") album_peak_in_block = b.size() + kv.first.size() + 1;
                b.insert(b.end(), e.begin(), e.end());
            }
            b.insert(b.begin(), {4, 0, 0, 0});
            // (the comment block is the first behind STREAMINFO: 4 + 4 + 34 bytes, then its own 4-byte header)
            gain_at = (long)(42 + 4 + gain_in_block); peak_at = (long)(42 + 4 + peak_in_block);
            album_gain_at = (long)(42 + 4 + album_gain_in_block); album_peak_at = (long)(42 + 4 + album_peak_in_block);
            blocks.push_back(std::move(b));
        }
        for (const TagPicture& p : pics) {
            std::vector<uint8_t> b = {6, 0, 0, 0};
            auto be32v = [&](uint32_t v) { uint8_t t[4]; put_be32(t, v); b.insert(b.end(), t, t + 4); };
            be32v(p.type);
            be32v((uint32_t)p.mime.size()); b.insert(b.end(), p.mime.begin(), p.mime.end());
            be32v((uint32_t)p.description.size()); b.insert(b.end(), p.description.begin(), p.description.end());
            be32v(0); be32v(0); be32v(0); be32v(0);                   // width, height, depth, colours: not parsed
            be32v((uint32_t)p.data.size()); b.insert(b.end(), p.data.begin(), p.data.end());
            if (b.size() - 4 < (1u << 24)) blocks.push_back(std::move(b));
        }
        for (auto& b : blocks) { const uint32_t n = (uint32_t)b.size() - 4; b[1] = (uint8_t)(n >> 16); b[2] = (uint8_t)(n >> 8); b[3] = (uint8_t)n; }
        if (!blocks.empty()) blocks.back()[0] |= 0x80;
        uint8_t h[4 + 4 + 34]; memset(h, 0, sizeof(h));
        memcpy(h, "fLaC", 4); h[4] = blocks.empty() ? 0x80 : 0x00; h[7] = 34;   // STREAMINFO
        if (fwrite(h, 1, sizeof(h), f) != sizeof(h)) return "short write";
        for (const auto& b : blocks) if (fwrite(b.data(), 1, b.size(), f) != b.size()) return "short write";
        return "";
    }
    // encodes the pending whole frames (and, at the end, the short last one) in batches, one thread per
    // frame of a batch, and writes them in order
    void drain(bool final) {
        if (encs.empty()) {
            (void)FlacFrameEnc::crc8_table(); (void)FlacFrameEnc::crc16_table();        // built before any thread runs
            unsigned hw = std::thread::hardware_concurrency();
            encs.resize(std::max(1u, std::min(16u, hw ? hw : 1u)));
        }
        const size_t per = (size_t)BS * ch;
        const size_t nfull = buf.size() / per, rem = buf.size() - nfull * per;
        std::vector<std::pair<size_t, uint32_t>> jobs;                   // (first sample, frames) of each FLAC frame
        for (size_t i = 0; i < nfull; ++i) jobs.push_back({i * per, BS});
        if (final && rem) jobs.push_back({nfull * per, (uint32_t)(rem / ch)});
        for (size_t j0 = 0; j0 < jobs.size(); j0 += encs.size()) {
            const size_t nb = std::min(encs.size(), jobs.size() - j0);
            std::vector<std::thread> th;
            for (size_t j = 1; j < nb; ++j)
                th.emplace_back([&, j] { encs[j].encode(buf.data() + jobs[j0 + j].first, jobs[j0 + j].second, ch, depth(), frame_no + (uint32_t)j, BS, effort); });
            encs[0].encode(buf.data() + jobs[j0].first, jobs[j0].second, ch, depth(), frame_no, BS, effort);
            for (auto& t : th) t.join();
            for (size_t j = 0; j < nb; ++j) {
                const std::vector<uint8_t>& o = encs[j].out;
                if (fwrite(o.data(), 1, o.size(), f) != o.size()) io_failed = true;
                if (o.size() < min_fs) min_fs = (uint32_t)o.size();
                if (o.size() > max_fs) max_fs = (uint32_t)o.size();
                frames += jobs[j0 + j].second;
            }
            frame_no += (uint32_t)nb;
        }
        buf.erase(buf.begin(), buf.begin() + (final ? buf.size() : nfull * per));
    }
    std::string write(const uint8_t* p, size_t nbytes) override {
        const size_t sb = bits == 16 ? 2 : 3;
        buf.reserve(buf.size() + nbytes / sb);
        for (size_t i = 0; i + sb <= nbytes; i += sb) {
            int32_t v = sb == 2 ? (int16_t)(p[i] | (p[i + 1] << 8)) : (int32_t)((p[i] | (p[i + 1] << 8) | (p[i + 2] << 16)) << 8) >> 8;
            if (bits == 20) v >>= 4;
            buf.push_back(v);
        }
        if (bits == 20) {                                                // MD5 runs over the 20-bit values as 3-byte integers
            for (size_t i = buf.size() - nbytes / sb; i < buf.size(); ++i) { const int32_t v = buf[i]; const uint8_t le[3] = {(uint8_t)v, (uint8_t)(v >> 8), (uint8_t)(v >> 16)}; md5.update(le, 3); }
        } else md5.update(p, nbytes / sb * sb);                          // 16/24-bit: the little-endian input as it is
        if (feed) { const std::string e = feed->write(p, nbytes); if (!e.empty()) return e; }
        if (buf.size() >= (size_t)BS * ch * 8) drain(false);
        return io_failed ? "short write" : "";
    }
    std::string write_frames(const uint8_t* p, size_t nbytes) override {
        raw_frames = true;
        return fwrite(p, 1, nbytes, f) == nbytes ? "" : "short write";
    }
    void set_frame_stats(uint64_t samples, uint64_t blocks, uint32_t min_bytes, uint32_t max_bytes) override {
        raw_frames = true;
        frames = samples;
        if (blocks) { min_fs = min_bytes; max_fs = max_bytes; }
    }
    std::string close() override {
        drain(true);
        uint8_t si[34]; memset(si, 0, sizeof(si));
        put_be16(si, BS); put_be16(si + 2, BS);
        si[4] = min_fs >> 16; si[5] = min_fs >> 8; si[6] = (uint8_t)min_fs; si[7] = max_fs >> 16; si[8] = max_fs >> 8; si[9] = (uint8_t)max_fs;
        const uint64_t v = ((uint64_t)rate << 44) | ((uint64_t)(ch - 1) << 41) | ((uint64_t)(depth() - 1) << 36) | (frames & 0xFFFFFFFFFull);
        for (int i = 0; i < 8; ++i) si[10 + i] = (uint8_t)(v >> (56 - 8 * i));
        if (!raw_frames) md5.finish(si + 18);
        else if (have_digest) memcpy(si + 18, digest, 16);               // (16 zero bytes otherwise: "not computed")
        fseek(f, 8, SEEK_SET); fwrite(si, 1, 34, f);
        std::string loud_error;
        if (replaygain) {
            // the sink's own measurement when it saw the samples, the GPU's otherwise (none: the placeholders stay)
            if (!raw_frames) {
                double tp = 0.0;
                loud_error = feed->finish(&loudness, true_peak ? &tp : nullptr); have_loudness = loud_error.empty();
                if (true_peak) loudness.peak = tp;
            }
            if (have_loudness) {
                const std::string g = replaygain_gain_text(loudness), p = replaygain_peak_text(loudness);
                fseek(f, gain_at, SEEK_SET); fwrite(g.data(), 1, g.size(), f);
                fseek(f, peak_at, SEEK_SET); fwrite(p.data(), 1, p.size(), f);
            }
            if (album && have_album) {
                const std::string g = replaygain_gain_text(album_loudness), p = replaygain_peak_text(album_loudness);
                fseek(f, album_gain_at, SEEK_SET); fwrite(g.data(), 1, g.size(), f);
                fseek(f, album_peak_at, SEEK_SET); fwrite(p.data(), 1, p.size(), f);
            }
        }
        if (fclose(f) != 0 || io_failed) return "close failed";
        if (!loud_error.empty()) return loud_error;
        return "";
    }
};

}  // namespace

std::string open_sink(OutputType type, const std::string& path, uint32_t channels, uint32_t rate, uint32_t bit_depth, PcmSink** out,
                      const std::vector<uint8_t>* id3, bool replaygain, bool true_peak, bool album) {
    *out = nullptr;
    if (true_peak && !replaygain) return "the true peak is written as REPLAYGAIN_TRACK_PEAK: it needs ReplayGain tags (--replaygain)";
    if (replaygain && type != OutputType::Flac) return "ReplayGain tags are written into FLAC files only; choose -o f";
    if (type == OutputType::Stdout) { *out = new RawSink(stdout); return ""; }
    if (type == OutputType::Flac && bit_depth == 32) return "FLAC cannot hold 32-bit float; choose 16, 20 or 24 bits";
    if (type == OutputType::Flac && rate > 655350) return "FLAC cannot describe this sample rate";
    if (type == OutputType::Flac && channels > 8) return "FLAC holds at most 8 channels";   // 4-bit channel assignment: 8..10 mean stereo decorrelation
    if (type == OutputType::Aiff && bit_depth == 32) return "AIFF cannot hold 32-bit float; use AIFC (C)";
    FILE* f = fopen(path.c_str(), "wb");
    if (!f) return "cannot create " + path;
    std::string err;
    if (type == OutputType::Wav) { auto* s = new WavSink(); if (id3) s->id3 = *id3; s->f = f; s->ch = channels; s->rate = rate; s->bits = bit_depth; err = s->begin(); *out = s; }
    else if (type == OutputType::Flac) { auto* s = new FlacSink(); if (id3) s->id3 = *id3; s->f = f; s->ch = channels; s->rate = rate; s->bits = bit_depth; s->replaygain = replaygain; s->true_peak = true_peak; s->album = replaygain && album; err = s->begin(); *out = s; }
    else { auto* s = new AiffSink(); if (id3) s->id3 = *id3; s->f = f; s->ch = channels; s->rate = rate; s->bits = bit_depth; s->aifc = type == OutputType::Aifc; err = s->begin(); *out = s; }
    return err;
}

}  // namespace d2dhost
