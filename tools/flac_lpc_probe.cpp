// flac_lpc_probe.cpp -- rule 13 of FLAC effort 12 (dsd2dxd_amd/csrc/flac/flac_lpc.h: from the autocorrelation to the quantised
// coefficients) on autocorrelations given on the command line, for tests/test_flac_lpc_cpu.py, which feeds it hand-made vectors that
// fire the branches windowed audio does not reach: the candidate dropped at sum |q| > 62 * 2^shift, the recursion stopped at
// !(err > 0).  CPU only:
//   g++ -O2 -std=c++17 -ffp-contract=off -Wall -o flac_lpc_probe flac_lpc_probe.cpp && ./flac_lpc_probe R0 R1 ... R12
// prints one line per order 4, 8, 12: "P none" or "P shift q1 ... qP".
#include <stdio.h>
#include <stdlib.h>

#include "../dsd2dxd_amd/csrc/flac/flac_lpc.h"

int main(int argc, char** argv) {
    using namespace d2dlpc;
    if (argc != MAX_ORDER + 2) { fprintf(stderr, "usage: flac_lpc_probe R0 .. R12\n"); return 2; }
    int64_t R[MAX_ORDER + 1];
    for (int l = 0; l <= MAX_ORDER; ++l) R[l] = strtoll(argv[1 + l], nullptr, 10);
    LpcCoefs c;
    lpc_coefficients(R, c);
    for (int s = 0; s < CANDIDATES; ++s) {
        const int P = 4 * (s + 1);
        if (!(c.valid >> s & 1u)) { printf("%d none\n", P); continue; }
        printf("%d %d", P, c.shift[s]);
        for (int j = 0; j < P; ++j) printf(" %d", c.q[s][j]);
        printf("\n");
    }
    return 0;
}
