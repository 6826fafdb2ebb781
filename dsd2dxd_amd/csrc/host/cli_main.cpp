// dsd2dxd_amd -- a small driver over include/rdsd2pcm.hpp with the reference CLI's flags
// (/root/reference/src/main.rs:40-133) for the conversion-relevant subset, plus:
//   probe  <file>...      print what the container readers see, as JSON (no GPU needed)
//   levels [opts] files   peak dBFS per file and overall (src/bin/dsd_levels/main.rs); --loudness adds each file's integrated loudness, --true-peak its true peak
//   -t S                  (convert and levels) not a reference letter: the 48 kHz multiples in two stages, D2D_FILTER_EQUIRIPPLE_CASCADE
//   tags [-a RATE] <file>...   the source's ID3v2 tag as the converted file would carry it, as JSON
//                         (text frames under their Vorbis names; -a applies the album suffix; no GPU needed)
//   verify <file.flac>... read back FLAC files the sinks here wrote: every frame is decoded (d2d_flac_decode_host) and the frame numbers,
//                         the sample count, the smallest and largest frame and -- where STREAMINFO has one -- the MD5 are checked; one
//                         line per file, a non-zero exit if any is bad (no GPU needed)
//   --downmix stereo|mono (convert and levels) fold a multichannel stream down inside the engine with the preset of the container's layout
//                         (raw input: by channel count, 4 = quad); --mix "g,g,..;g,g,.." an explicit matrix of decimal gains, a row per
//                         output channel (Rdsd2Pcm::set_downmix / set_mix); `levels --downmix` reports the folded peak
// It is not the reference's CLI (logging, progress bars, Rayon pool are out of scope).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <cmath>
#include <string>
#include <vector>

#include "../../../include/dsd2dxd_amd.h"
#include "../../../include/rdsd2pcm.hpp"
#include "../flac/flac_parse.h"
#include "../mix/d2d_mix_text.h"
#include "dsd_reader.h"
#include "id3_tag.h"
#include "md5.h"

using namespace rdsd2pcm;
static std::atomic<bool> CANCEL_FLAG{false};

static int probe_main(int argc, char** argv) {
    printf("[");
    for (int i = 0; i < argc; ++i) {
        d2dhost::DsdInfo o;
        std::string err = d2dhost::probe(argv[i], o);
        printf("%s{\"path\": \"%s\", \"error\": \"%s\", \"format\": \"%s\", \"channels\": %u, \"dsd_rate\": %u, \"planar\": %s, "
               "\"msb_first\": %s, \"block_size\": %u, \"bytes_per_channel\": %llu, \"sample_count\": %llu, \"data_offset\": %llu, "
               "\"data_bytes\": %llu, \"metadata_offset\": %llu, \"metadata_truncated\": %s, \"warning\": \"%s\"}",
               i ? ", " : "", argv[i], err.c_str(), o.format == d2dhost::DsdFileFormat::Dsf ? "dsf" : o.format == d2dhost::DsdFileFormat::Dff ? "dff" : "other",
               o.channels, o.dsd_rate, o.planar ? "true" : "false", o.msb_first ? "true" : "false", o.block_size,
               (unsigned long long)o.bytes_per_channel, (unsigned long long)o.sample_count, (unsigned long long)o.data_offset,
               (unsigned long long)o.data_bytes, (unsigned long long)o.metadata_offset, o.metadata_truncated ? "true" : "false", o.warning.c_str());
    }
    printf("]\n");
    return 0;
}

static std::string json_escape(const std::string& s) {
    std::string o;
    for (unsigned char c : s) {
        if (c == '"' || c == '\\') { o += '\\'; o += (char)c; }
        else if (c < 0x20) { char b[8]; snprintf(b, sizeof(b), "\\u%04x", c); o += b; }
        else o += (char)c;
    }
    return o;
}

static int tags_main(int argc, char** argv) {
    uint32_t append_rate = 0;
    int i = 0;
    if (argc >= 2 && !strcmp(argv[0], "-a")) { append_rate = (uint32_t)strtoul(argv[1], 0, 10); i = 2; }
    printf("[");
    for (bool first = true; i < argc; ++i, first = false) {
        d2dhost::DsdInfo o;
        std::string err = d2dhost::probe(argv[i], o), warn;
        std::vector<uint8_t> tag;
        if (err.empty()) err = d2dhost::read_source_tag(argv[i], o, tag, warn);
        bool album_edited = false;
        if (!tag.empty() && append_rate) album_edited = d2dhost::append_to_album(tag, d2dhost::album_rate_suffix(append_rate));
        std::vector<std::pair<std::string, std::string>> fields;
        std::vector<d2dhost::TagPicture> pics;
        d2dhost::tag_to_vorbis(tag, fields, pics);
        printf("%s{\"path\": \"%s\", \"error\": \"%s\", \"warning\": \"%s\", \"tag_bytes\": %zu, \"album_edited\": %s, \"pictures\": %zu, \"fields\": {",
               first ? "" : ", ", json_escape(argv[i]).c_str(), json_escape(err).c_str(), json_escape(warn).c_str(), tag.size(),
               album_edited ? "true" : "false", pics.size());
        for (size_t k = 0; k < fields.size(); ++k)
            printf("%s\"%s\": \"%s\"", k ? ", " : "", json_escape(fields[k].first).c_str(), json_escape(fields[k].second).c_str());
        printf("}}");
    }
    printf("]\n");
    return 0;
}

// ---- verify: a FLAC file of the sinks here, read back ------------------------------------------------------------------------------
static const char* const REASONS[] = {"none", "SIZE", "HEADER", "CRC8", "CRC16", "UNSUPPORTED", "SYNTAX", "LENGTH", "SAMPLES"};

// takes the samples of a frame and drops them: the walk below wants the frames' sizes only
struct NoSamples {
    int32_t store[2 * d2dparse::MAX_LPC_ORDER];
    void begin(uint32_t, uint32_t) {}
    bool put(uint32_t, int32_t) { return true; }
    int32_t& hist(uint32_t k) { return store[k]; }
    int32_t& coef(uint32_t k) { return store[d2dparse::MAX_LPC_ORDER + k]; }
};

// "" when the file is good (*no_md5: its STREAMINFO has no MD5), else what is wrong with it
static std::string verify_file(const char* path, bool* no_md5) {
    FILE* f = fopen(path, "rb");
    if (!f) return "cannot open";
    std::vector<uint8_t> file;
    uint8_t chunk[1 << 16];
    for (size_t n; (n = fread(chunk, 1, sizeof(chunk), f)) > 0;) file.insert(file.end(), chunk, chunk + n);
    fclose(f);
    if (file.size() < 42 || memcmp(file.data(), "fLaC", 4) || (file[4] & 0x7F) != 0 || file[5] || file[6] || file[7] != 34) return "not a FLAC file that begins with STREAMINFO";
    const uint8_t* si = file.data() + 8;
    size_t pos = 4;
    for (bool last = false; !last;) {                                 // metadata blocks are skipped by their length
        if (pos + 4 > file.size()) return "metadata runs past the end of the file";
        last = file[pos] & 0x80;
        pos += 4 + (((size_t)file[pos + 1] << 16) | ((size_t)file[pos + 2] << 8) | file[pos + 3]);
    }
    if (pos > file.size()) return "metadata runs past the end of the file";
    const uint32_t block_min = (si[0] << 8) | si[1], block_max = (si[2] << 8) | si[3];
    const uint32_t frame_min = (si[4] << 16) | (si[5] << 8) | si[6], frame_max = (si[7] << 16) | (si[8] << 8) | si[9];
    uint64_t v = 0;
    for (int i = 0; i < 8; ++i) v = (v << 8) | si[10 + i];
    const uint32_t channels = (uint32_t)((v >> 41) & 7) + 1, depth = (uint32_t)((v >> 36) & 31) + 1;
    const uint64_t total = v & 0xFFFFFFFFFull;
    if (block_min != D2D_FLAC_BLOCK || block_max != D2D_FLAC_BLOCK) return "not a stream of 4096-sample blocks";
    if (depth != 16 && depth != 20 && depth != 24) return "not 16, 20 or 24 bits";
    const uint8_t* audio = file.data() + pos;
    const size_t bytes = file.size() - pos, frame_bytes = (size_t)channels * (depth == 16 ? 2 : 3);
    std::vector<uint8_t> pcm((size_t)(total + D2D_FLAC_BLOCK) * frame_bytes);
    size_t frames_out = 0;
    d2d_flac_check check{};
    const int rc = d2d_flac_decode_host(channels, depth, audio, bytes, 0, pcm.data(), pcm.size(), &frames_out, &check);
    if (rc == D2D_ERR_CAPACITY) return "the frames hold more samples than STREAMINFO's " + std::to_string(total);
    if (rc != D2D_OK) return d2d_flac_error();
    if (check.bad_blocks) return "block " + std::to_string(check.first_bad_block) + ": " + REASONS[check.first_bad_reason < 9 ? check.first_bad_reason : 0];
    if (frames_out != total) return "the frames hold " + std::to_string(frames_out) + " samples, STREAMINFO says " + std::to_string(total);
    // the frames' sizes: the same parser once more, without the samples
    uint16_t tab[256];
    for (uint32_t i = 0; i < 256; ++i) tab[i] = (uint16_t)d2dparse::crc16_entry(i);
    uint32_t smallest = 0, largest = 0;
    NoSamples sig;
    size_t off = 0;
    for (uint32_t b = 0; off < bytes; ++b) {
        d2dparse::Header h{0, 0, 0};
        uint32_t size = 0;
        const uint32_t avail = (uint32_t)std::min<size_t>(bytes - off, (size_t)1 << 20);
        const uint32_t reason = d2dparse::parse_frame(audio + off, avail, false, d2dparse::Expect{channels, depth, 0, b}, tab, sig, h, &size);
        if (reason) return "block " + std::to_string(b) + ": " + REASONS[reason];
        smallest = b ? std::min(smallest, size) : size; largest = std::max(largest, size);
        off += size;
    }
    if (smallest != frame_min || largest != frame_max)
        return "frames of " + std::to_string(smallest) + " to " + std::to_string(largest) + " bytes, STREAMINFO says " + std::to_string(frame_min) + " to " + std::to_string(frame_max);
    static const uint8_t zero[16] = {};
    *no_md5 = !memcmp(si + 18, zero, 16);
    if (*no_md5) return "";
    d2dhost::Md5 md5;                                               // over the samples as little-endian whole-byte integers, interleaved
    if (depth == 20) {
        for (size_t i = 0; i < frames_out * channels; ++i) {
            const int32_t s = (int32_t)((uint32_t)(pcm[3 * i] | (pcm[3 * i + 1] << 8) | (pcm[3 * i + 2] << 16)) << 8) >> 12;
            const uint8_t le[3] = {(uint8_t)s, (uint8_t)(s >> 8), (uint8_t)(s >> 16)};
            md5.update(le, 3);
        }
    } else md5.update(pcm.data(), frames_out * frame_bytes);
    uint8_t digest[16];
    md5.finish(digest);
    return memcmp(digest, si + 18, 16) ? "the decoded samples do not have STREAMINFO's MD5" : "";
}

static int verify_main(int argc, char** argv) {
    if (argc == 0) { fprintf(stderr, "verify: no files\n"); return 2; }
    int bad = 0;
    for (int i = 0; i < argc; ++i) {
        bool no_md5 = false;
        const std::string err = verify_file(argv[i], &no_md5);
        if (!err.empty()) { printf("%s: BAD: %s\n", argv[i], err.c_str()); ++bad; }
        else printf("%s: %s\n", argv[i], no_md5 ? "ok (no MD5 in STREAMINFO)" : "ok");
    }
    return bad ? 1 : 0;
}

int main(int argc, char** argv) {
    if (argc >= 2 && !strcmp(argv[1], "probe")) return probe_main(argc - 2, argv + 2);
    if (argc >= 2 && !strcmp(argv[1], "verify")) return verify_main(argc - 2, argv + 2);
    if (argc >= 2 && !strcmp(argv[1], "tags")) return tags_main(argc - 2, argv + 2);
    bool levels = false;
    int ai = 1;
    if (argc >= 2 && !strcmp(argv[1], "levels")) { levels = true; ai = 2; }
    else if (argc >= 2 && !strcmp(argv[1], "convert")) ai = 2;
    // defaults of the reference CLI (src/main.rs:50-110)
    std::string out_dir; bool have_out_dir = false;
    size_t channels = 2, bit_depth = 24; char fmt = 'I', filt = 'E', endian = 'M', dither = 0, output = 'S';
    uint32_t block = 4096, rate = 352800, inrate = 1; double level = 0.0; bool append = false, recurse = false, quiet = false;
    int device = 0; unsigned long long seed = 0; uint32_t tap_bits = 0; bool gpu_flac = false, flac_verify = false, flac_md5 = false, replaygain = false, loudness = false, true_peak = false, album = false; int flac_effort = 0;
    uint32_t downmix = 0; std::vector<int32_t> mix; uint32_t mix_rows = 0, mix_cols = 0;
    std::vector<std::string> files;
    for (; ai < argc; ++ai) {
        std::string a = argv[ai];
        auto val = [&]() -> const char* { if (ai + 1 >= argc) { fprintf(stderr, "missing value for %s\n", a.c_str()); exit(2); } return argv[++ai]; };
        if (a == "-p" || a == "--path") { out_dir = val(); have_out_dir = true; }
        else if (a == "-c" || a == "--channels") channels = strtoul(val(), 0, 10);
        else if (a == "-f" || a == "--fmt") fmt = val()[0];
        else if (a == "-b" || a == "--bitdepth") bit_depth = strtoul(val(), 0, 10);
        else if (a == "-t" || a == "--filttype") filt = val()[0];
        else if (a == "-e" || a == "--endianness") endian = val()[0];
        else if (a == "-s" || a == "--bs") block = (uint32_t)strtoul(val(), 0, 10);
        else if (a == "-d" || a == "--dither") dither = val()[0];
        else if (a == "-r" || a == "--rate") rate = (uint32_t)strtoul(val(), 0, 10);
        else if (a == "-i" || a == "--inrate") inrate = (uint32_t)strtoul(val(), 0, 10);
        else if (a == "-o" || a == "--output") output = val()[0];
        else if (a == "-l" || a == "--level") level = atof(val());
        else if (a.rfind("--level=", 0) == 0) level = atof(a.c_str() + 8);
        else if (a == "-a" || a == "--append") append = true;
        else if (a == "-R" || a == "--recurse") recurse = true;
        else if (a == "-q" || a == "--quiet") quiet = true;
        else if (a == "-v" || a == "--verbose") {}
        else if (a == "--device") device = atoi(val());
        else if (a == "--seed") seed = strtoull(val(), 0, 10);
        else if (a == "--tap-bits") tap_bits = (uint32_t)strtoul(val(), 0, 10);
        else if (a == "--gpu-flac") gpu_flac = true;               // -o f only: encode the frames on the GPU (Rdsd2Pcm::set_gpu_flac)
        else if (a == "--flac-effort") flac_effort = atoi(val());  // -o f only: 0 (default), 1, the search, or 12, the search with LPC (Rdsd2Pcm::set_flac_effort)
        else if (a == "--flac-verify") flac_verify = true;         // --gpu-flac -o f only: check every frame against its PCM on the GPU before it is written (Rdsd2Pcm::set_flac_verify)
        else if (a == "--flac-md5") flac_md5 = true;               // --gpu-flac -o f only: hash the samples on the GPU and fill in STREAMINFO's MD5 (Rdsd2Pcm::set_flac_md5)
        else if (a == "--replaygain") replaygain = true;           // -o f only, with or without --gpu-flac: measure BS.1770 loudness and the sample peak and write the REPLAYGAIN_* fields (Rdsd2Pcm::set_replaygain)
        else if (a == "--loudness") loudness = true;               // levels only: integrated loudness behind each file's peak (Rdsd2Pcm::set_loudness)
        else if (a == "--true-peak") true_peak = true;             // convert with --replaygain: REPLAYGAIN_TRACK_PEAK is the true peak; levels: each file's true peak in dBTP (Rdsd2Pcm::set_true_peak)
        else if (a == "--album") album = true;                     // convert -o f only: all inputs of the command are one album (Rdsd2Pcm::convert_album): with --gpu-flac one engine for all, with --replaygain the REPLAYGAIN_ALBUM_* fields
        else if (a == "--downmix") {                               // fold down with the preset of the layout (Rdsd2Pcm::set_downmix)
            const std::string t = val();
            downmix = t == "stereo" ? 2u : t == "mono" ? 1u : 0u;
            if (!downmix) { fprintf(stderr, "ERROR: --downmix takes stereo or mono\n"); return 2; }
        } else if (a == "--mix") {                                 // an explicit matrix, decimal gains rounded to Q15 (Rdsd2Pcm::set_mix)
            std::string err;
            if (!d2d::parse_mix_text(val(), mix, mix_rows, mix_cols, err)) { fprintf(stderr, "ERROR: --mix: %s\n", err.c_str()); return 2; }
        }
        else files.push_back(a);
    }
    if (album && (levels || tolower(output) != 'f')) {
        fprintf(stderr, "ERROR: --album converts the inputs of the command as one album of FLAC files: it needs `convert` and -o f\n");
        return 2;
    }
    if (true_peak && !levels && !replaygain) {
        fprintf(stderr, "ERROR: --true-peak writes REPLAYGAIN_TRACK_PEAK as a true peak: on a conversion it needs --replaygain\n");
        return 2;
    }
    if (replaygain && (levels || tolower(output) != 'f')) {
        fprintf(stderr, "ERROR: --replaygain writes its tags into FLAC files only: it needs -o f\n");
        return 2;
    }
    if (loudness && !levels) {
        fprintf(stderr, "ERROR: --loudness belongs to `levels`; a conversion measures with --replaygain\n");
        return 2;
    }
    if (flac_md5 && !(gpu_flac && tolower(output) == 'f')) {
        fprintf(stderr, "ERROR: --flac-md5 hashes the samples --gpu-flac encodes: it needs --gpu-flac and -o f\n");
        return 2;
    }
    if (flac_verify && !(gpu_flac && tolower(output) == 'f')) {
        fprintf(stderr, "ERROR: --flac-verify checks the frames --gpu-flac encodes: it needs --gpu-flac and -o f\n");
        return 2;
    }
    if (downmix && mix_rows) {
        fprintf(stderr, "ERROR: --downmix and --mix both set the engine's one matrix: give one of them\n");
        return 2;
    }
    if (files.empty()) files.push_back("-");
    try {
        // char -> enum exactly as src/main.rs:165-214 (unknown endianness/filter/output fall back, unknown dither/format fail)
        if (!dither) dither = bit_depth == 32 ? 'F' : 'T';
        DitherType dt;
        switch (tolower(dither)) { case 't': dt = DitherType::TPDF; break; case 'r': dt = DitherType::Rectangular; break;
            case 'f': dt = DitherType::FPD; break; case 'x': dt = DitherType::None; break;
            case 'n': dt = DitherType::NoiseShaped; break;                 // extension: noise-shaped TPDF
            default: throw std::runtime_error("Invalid dither type; must be T, R, F, or X"); }
        FmtType ft;
        switch (tolower(fmt)) { case 'i': ft = FmtType::Interleaved; break; case 'p': ft = FmtType::Planar; break;
            default: throw std::runtime_error("Invalid format; must be I (interleaved) or P (planar)"); }
        Endianness en = tolower(endian) == 'l' ? Endianness::LsbFirst : Endianness::MsbFirst;
        FilterType fl = toupper(filt) == 'X' ? FilterType::XLD : toupper(filt) == 'D' ? FilterType::Dsd2Pcm : toupper(filt) == 'C' ? FilterType::Chebyshev :
                        toupper(filt) == 'S' ? FilterType::EquirippleCascade : FilterType::Equiripple;      // S: extension, the 48 kHz multiples in two stages
        OutputType ot = tolower(output) == 'a' ? OutputType::Aiff : tolower(output) == 'c' ? OutputType::Aifc : tolower(output) == 'w' ? OutputType::Wav : tolower(output) == 'f' ? OutputType::Flac : OutputType::Stdout;
        bool has_stdin = false;
        std::vector<std::string> paths;
        for (auto& f : files) { if (f == "-") has_stdin = true; else paths.push_back(f); }
        std::vector<std::string> expanded = find_dsd_files(paths, recurse);
        if (has_stdin) expanded.insert(expanded.begin(), "-");
        const bool half = rate == 44100 || rate == 48000;                  // extension: the halved rates, through the exact 2:1 decimator behind the FIR (Rdsd2Pcm::create_half)
        float overall = -INFINITY;
        std::vector<Rdsd2Pcm> tracks;                                      // --album: every input, converted together behind the loop
        for (auto& path : expanded) {
            const bool is_stdin = path == "-";
            std::optional<std::string> od; if (have_out_dir) od = out_dir;
            std::optional<std::string> ip; if (!is_stdin) ip = path;
            if (levels) {
                // (the reference's level check is always the equiripple filter, whatever -t says; -t S chooses which of its two definitions)
                const FilterType lf = fl == FilterType::EquirippleCascade ? fl : FilterType::Equiripple;
                Rdsd2Pcm lib = half ? Rdsd2Pcm::new_level_check_half(rate, ip, ft, en, channels, block, inrate, lf)
                                    : Rdsd2Pcm::new_level_check(rate, ip, ft, en, channels, block, inrate, lf);
                lib.set_device(device); lib.set_loudness(loudness); lib.set_true_peak(true_peak);
                if (downmix) lib.set_downmix(downmix);
                if (mix_rows) lib.set_mix(mix_rows, mix);
                float db = lib.check_level(CANCEL_FLAG);
                if (!loudness) printf("%s: %.4f dBFS", lib.file_name().c_str(), db);
                else if (lib.loudness_valid()) printf("%s: %.4f dBFS, %.2f LUFS", lib.file_name().c_str(), db, lib.loudness_lufs());
                else printf("%s: %.4f dBFS, -inf LUFS", lib.file_name().c_str(), db);
                if (true_peak) printf(", %.4f dBTP", lib.true_peak_dbtp());
                printf("\n");
                if (!std::isnan(db) && db > overall) overall = db;          // dsd_levels/main.rs:184-202 skips NaN
                continue;
            }
            const bool container = !is_stdin && DsdFileFormat::from(path).is_container();
            Rdsd2Pcm lib = container ? (half ? Rdsd2Pcm::from_container_half(bit_depth, ot, level, rate, od, dt, fl, append, ".", path)
                                             : Rdsd2Pcm::from_container(bit_depth, ot, level, rate, od, dt, fl, append, ".", path))
                                     : (half ? Rdsd2Pcm::create_half(bit_depth, ot, level, rate, od, dt, ft, en, inrate, block, channels, fl, append, ".", ip)
                                             : Rdsd2Pcm::create(bit_depth, ot, level, rate, od, dt, ft, en, inrate, block, channels, fl, append, ".", ip));
            lib.set_device(device); lib.set_seed(seed); lib.set_tap_bits(tap_bits); lib.set_gpu_flac(gpu_flac); lib.set_flac_effort(flac_effort); lib.set_flac_verify(flac_verify); lib.set_flac_md5(flac_md5); lib.set_replaygain(replaygain); lib.set_true_peak(true_peak);
            if (downmix) lib.set_downmix(downmix);
            if (mix_rows) lib.set_mix(mix_rows, mix);
            if (album) { tracks.push_back(std::move(lib)); continue; }
            lib.do_conversion(CANCEL_FLAG);
            if (!quiet && !lib.warnings().empty()) fprintf(stderr, "WARNING: %s: %s\n", lib.file_name().c_str(), lib.warnings().c_str());
            if (!quiet && lib.audio_seconds() > 0)
                fprintf(stderr, "DSP speed for %s: %.2fx\n", lib.file_name().c_str(), lib.audio_seconds() / std::max(lib.dsp_seconds(), 1e-9));
        }
        if (album) {
            Rdsd2Pcm::convert_album(tracks, CANCEL_FLAG);
            for (auto& lib : tracks)
                if (!quiet && !lib.warnings().empty()) fprintf(stderr, "WARNING: %s: %s\n", lib.file_name().c_str(), lib.warnings().c_str());
            if (!quiet && tracks[0].audio_seconds() > 0)
                fprintf(stderr, "DSP speed for the album of %zu: %.2fx\n", tracks.size(), tracks[0].audio_seconds() / std::max(tracks[0].dsp_seconds(), 1e-9));
        }
        if (levels) printf("Highest peak: %.4f dBFS\n", overall);
    } catch (const std::exception& ex) {
        fprintf(stderr, "ERROR: %s\n", ex.what());
        return 1;
    }
    return 0;
}
