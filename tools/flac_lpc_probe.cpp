// flac_lpc_probe.cpp -- rule 13 of FLAC effort 12 (dsd2dxd_amd/csrc/flac/flac_lpc.h: from the autocorrelation to the quantised
// coefficients) on autocorrelations given on the command line or in a file, for tests/test_flac_lpc_cpu.py and
// tests/test_flac_search_edges_cpu.py, which feed it hand-made vectors that fire the branches windowed audio does not reach: the
// candidate dropped at sum |q| > 62 * 2^shift, the recursion stopped at !(err > 0).  CPU only:
//   g++ -O2 -std=c++17 -ffp-contract=off -Wall -o flac_lpc_probe flac_lpc_probe.cpp
//   ./flac_lpc_probe R0 R1 ... R12          one vector
//   ./flac_lpc_probe FILE                   many: whitespace-separated integers, thirteen per vector
// prints per vector, in the order given, one line per order 4, 8, 12: "P none" or "P shift q1 ... qP".
// tools/flac_lpc_probe_gpu.hip is the same program with the routine run on the device.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../dsd2dxd_amd/csrc/flac/flac_lpc.h"

int main(int argc, char** argv) {
    using namespace d2dlpc;
    std::vector<int64_t> R;
    if (argc == MAX_ORDER + 2) {
        for (int l = 0; l <= MAX_ORDER; ++l) R.push_back(strtoll(argv[1 + l], nullptr, 10));
    } else if (argc == 2) {
        FILE* f = fopen(argv[1], "r");
        if (!f) { fprintf(stderr, "flac_lpc_probe: cannot open %s\n", argv[1]); return 2; }
        long long v;
        while (fscanf(f, "%lld", &v) == 1) R.push_back(v);
        fclose(f);
        if (R.empty() || R.size() % (MAX_ORDER + 1)) { fprintf(stderr, "flac_lpc_probe: %s: not a multiple of thirteen integers\n", argv[1]); return 2; }
    } else {
        fprintf(stderr, "usage: flac_lpc_probe R0 .. R12 | flac_lpc_probe FILE\n");
        return 2;
    }
    for (size_t v = 0; v < R.size() / (MAX_ORDER + 1); ++v) {
        LpcCoefs c;
        lpc_coefficients(&R[v * (MAX_ORDER + 1)], c);
        for (int s = 0; s < CANDIDATES; ++s) {
            const int P = 4 * (s + 1);
            if (!(c.valid >> s & 1u)) { printf("%d none\n", P); continue; }
            printf("%d %d", P, c.shift[s]);
            for (int j = 0; j < P; ++j) printf(" %d", c.q[s][j]);
            printf("\n");
        }
    }
    return 0;
}
