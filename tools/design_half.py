#!/usr/bin/env python3
"""Design and freeze the 2:1 decimator behind the FIR: filters/half_table.inc.

One table serves 88.2 -> 44.1 kHz and 96 -> 48 kHz.  Edges as fractions of the input rate: pass band up to 0.22676 (20 kHz at
88.2 kHz), stop band from 0.25 (the new Nyquist: nothing folds back below its last 2 kHz).  An equiripple design of NT taps,
rounded to q * 2^-T; the centre tap then takes the rounding's remainder so that sum q = 2^T exactly (a constant comes out as
itself).  The conditions the committed integers must meet (tests/test_half_cpu.py checks them on the file, not on this script):

    NT odd, symmetric;  sum q = 2^T;  sum |q| < 2^28;  pass-band ripple <= 1e-4 dB;  stop band <= -126 dB   (FFT of 2^17 points)

Run:  python tools/design_half.py            -> writes filters/half_table.inc
      python tools/design_half.py --check    -> measures the committed file
"""
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATH = os.path.join(ROOT, "filters", "half_table.inc")
NT, T = 383, 26
F_PASS, F_STOP, STOP_WEIGHT = 0.22676, 0.25, 30.0


def design():
    import scipy.signal as sg
    h = sg.remez(NT, [0, F_PASS, F_STOP, 0.5], [1, 0], weight=[1, STOP_WEIGHT], fs=1, maxiter=200)
    h = 0.5 * (h + h[::-1])                              # exactly symmetric before rounding
    q = [int(v) for v in np.round(h / h.sum() * (1 << T))]
    q[NT // 2] += (1 << T) - sum(q)                      # unity at DC, exactly
    return q


def measure(q, t, nfft=1 << 17):
    """(pass-band ripple in dB, peak to peak about 0 dB as the larger deviation; stop-band peak in dB) of the integers."""
    H = np.abs(np.fft.rfft(np.array(q, dtype=np.float64) / float(1 << t), nfft))
    f = np.arange(H.size) / nfft
    pb = 20 * np.log10(H[f <= F_PASS])
    sb = 20 * np.log10(np.maximum(H[f >= F_STOP], 1e-300))
    return float(np.max(np.abs(pb))), float(np.max(sb))


def parse(path=PATH):
    text = open(path).read()
    nt = int(re.search(r"D2D_HALF_NT\s*=\s*(\d+)", text).group(1))
    t = int(re.search(r"D2D_HALF_T\s*=\s*(\d+)", text).group(1))
    body = re.search(r"D2D_HALF_TAPS\[[^\]]*\]\s*=\s*\{([^}]*)\}", text).group(1)
    q = [int(v) for v in body.replace("\n", " ").split(",") if v.strip()]
    assert len(q) == nt
    return nt, t, q


def write(q):
    lines = ["// half_table.inc -- the 2:1 decimator behind the FIR (DESIGN section 4.5c), frozen by tools/design_half.py.  Do not edit.",
             "// h[j] = q[j] * 2^-T: NT taps, symmetric, sum q = 2^T, sum |q| < 2^28; pass band to 0.22676, stop band from 0.25 of the input rate.",
             "#pragma once", "#include <stdint.h>", "",
             "enum { D2D_HALF_NT = %d, D2D_HALF_T = %d };" % (len(q), T),
             "#ifdef __cplusplus", "#define D2D_HALF_CONST constexpr", "#else", "#define D2D_HALF_CONST const", "#endif",
             "static D2D_HALF_CONST int32_t D2D_HALF_TAPS[D2D_HALF_NT] = {"]
    for i in range(0, len(q), 12):
        lines.append("  " + ", ".join(str(v) for v in q[i:i + 12]) + ",")
    lines.append("};")
    with open(PATH, "w") as f:
        f.write("\n".join(lines) + "\n")


def report(nt, t, q):
    ripple, stop = measure(q, t)
    sa = sum(abs(v) for v in q)
    print("NT %d  T %d  symmetric %s  sum q - 2^T = %d  sum|q| = 2^%.3f" % (nt, t, q == q[::-1], sum(q) - (1 << t), np.log2(sa)))
    print("pass-band deviation %.7f dB   stop band %.2f dB" % (ripple, stop))
    ok = nt % 2 == 1 and q == q[::-1] and sum(q) == 1 << t and sa < 1 << 28 and ripple <= 1e-4 and stop <= -126.0
    print("conditions", "hold" if ok else "FAIL")
    return ok


if __name__ == "__main__":
    if "--check" not in sys.argv[1:]:
        write(design())
    sys.exit(0 if report(*parse()) else 1)
