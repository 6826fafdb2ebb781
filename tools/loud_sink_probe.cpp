// loud_sink_probe.cpp -- the FLAC sink of the host driver (dsd2dxd_amd/csrc/host/pcm_sink.cpp) without an engine: packed PCM from a file
// goes through open_sink / write / close, with or without `replaygain`, so that tests/test_loudness_cpu.py can hold the file the host
// path writes -- its REPLAYGAIN_* fields, the source's other fields, `verify` -- without a GPU:
//   g++ -O2 -std=c++17 -ffp-contract=off -o loud_sink_probe tools/loud_sink_probe.cpp dsd2dxd_amd/csrc/host/pcm_sink.cpp
//       dsd2dxd_amd/csrc/host/id3_tag.cpp dsd2dxd_amd/csrc/loud/d2d_loud_host.cpp dsd2dxd_amd/csrc/flac/d2d_flac_host.cpp -lpthread
//   ./loud_sink_probe OUT.flac CHANNELS DEPTH RATE REPLAYGAIN(0|1|2|3) PCM_FILE WRITE_BYTES [ID3_FILE]
// REPLAYGAIN 2: `replaygain` and `true_peak` (tests/test_true_peak_cpu.py); 3: `true_peak` alone, which open_sink refuses.
// WRITE_BYTES: the size of one write() call, rounded down to whole frames (the sink's result must not depend on it).
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "../dsd2dxd_amd/csrc/host/pcm_sink.h"

static std::vector<uint8_t> slurp(const char* path) {
    std::vector<uint8_t> v;
    FILE* f = fopen(path, "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", path); exit(2); }
    uint8_t buf[1 << 16];
    for (size_t n; (n = fread(buf, 1, sizeof(buf), f)) > 0;) v.insert(v.end(), buf, buf + n);
    fclose(f);
    return v;
}

int main(int argc, char** argv) {
    if (argc < 8) { fprintf(stderr, "usage: loud_sink_probe OUT CHANNELS DEPTH RATE REPLAYGAIN PCM_FILE WRITE_BYTES [ID3_FILE]\n"); return 2; }
    const uint32_t ch = (uint32_t)atoi(argv[2]), depth = (uint32_t)atoi(argv[3]), rate = (uint32_t)atoi(argv[4]);
    const bool replaygain = atoi(argv[5]) == 1 || atoi(argv[5]) == 2, true_peak = atoi(argv[5]) >= 2;
    const std::vector<uint8_t> pcm = slurp(argv[6]);
    const size_t fb = (size_t)ch * (depth == 16 ? 2 : 3);
    const size_t step = std::max(fb, (size_t)atol(argv[7]) / fb * fb);
    std::vector<uint8_t> tag;
    if (argc > 8) tag = slurp(argv[8]);
    d2dhost::PcmSink* sink = nullptr;
    std::string err = d2dhost::open_sink(d2dhost::OutputType::Flac, argv[1], ch, rate, depth, &sink, &tag, replaygain, true_peak);
    for (size_t at = 0; err.empty() && at < pcm.size(); at += step) err = sink->write(pcm.data() + at, std::min(step, pcm.size() - at));
    if (sink) { const std::string ce = sink->close(); if (err.empty()) err = ce; }
    delete sink;
    if (!err.empty()) { printf("ERROR: %s\n", err.c_str()); return 1; }
    printf("ok\n");
    return 0;
}
