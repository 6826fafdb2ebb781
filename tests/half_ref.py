"""The reference of the 2:1 decimator behind the FIR, built on the oracle and nothing of the product:

  * mix_ref.exact_sums gives the oracle's exact integer FIR sums at the DOUBLED rate; they are shifted to the table's own S, which the
    caller states (28 / 29 / 30 for *_M32 / *_M64 / *_M128, 28 / 29 for P_1_96000 / P_2_96000);
  * steps 1-2 in integers, with the taps parsed from the committed filters/half_table.inc:
        v[k] = sum_j q[j] x[2k - j],  w[k] = (v[k] + 2^(T-1)) >> T       (x[i] = 0 for i < 0)
    in Python integers, or -- for the long streams of the GPU tests -- in numpy int64 after asserting the bound that keeps int64 exact
    (max |x| * sum |q| < 2^62; tests/test_half_cpu.py holds the two forms together);
  * y[k] = w[k] * 2^-S and mix_ref.emit (the oracle's emit_sample restated) on (seed, channel, k) for step 3.

Shared by tests/test_half_cpu.py, tests/test_gpu_half.py and tests/test_gpu_half_cli.py."""
import math
import os
import re

import numpy as np

import mix_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "filters", "half_table.inc")

# the S of the table that serves (dsd_rate, final rate, filter) at the doubled rate, as filters/filter_tables.inc names them
SCALE = {(1, 44100, "E"): 28, (2, 44100, "E"): 29, (4, 44100, "E"): 30, (1, 44100, "X"): 28, (2, 44100, "C"): 29,
         (1, 48000, "E"): 28, (2, 48000, "E"): 29}

_TAPS = None


def taps():
    """(q as a list of Python integers, T) from the committed table file"""
    global _TAPS
    if _TAPS is None:
        text = open(TABLE).read()
        nt = int(re.search(r"D2D_HALF_NT\s*=\s*(\d+)", text).group(1))
        t = int(re.search(r"D2D_HALF_T\s*=\s*(\d+)", text).group(1))
        body = re.search(r"D2D_HALF_TAPS\[[^\]]*\]\s*=\s*\{([^}]*)\}", text).group(1)
        q = [int(v) for v in body.replace("\n", " ").split(",") if v.strip()]
        assert len(q) == nt
        _TAPS = (q, t)
    return _TAPS


def frames_after(n):
    return (n + 1) >> 1


def doubled(kw):
    """the oracle's arguments of the FIR a halved engine of `kw` runs: the same at twice the rate"""
    return dict(kw, output_rate=2 * kw["output_rate"])


def sums_at(O, kw, bufs, S):
    """the exact sums of the stream `bufs` at the doubled rate of kw, on the table's grid 2^-S: an int64 array (channels, n)"""
    X, s0 = mix_ref.exact_sums(O, doubled(kw), bufs)
    assert s0 <= S, (s0, S)
    X = X << (S - s0)
    assert np.all(np.abs(X) < 1 << 31)
    return X


def half_w(line, first, exact_python=None):
    """w[k] of the frames first <= 2k < first + n of ONE channel.  line: NT - 1 carried sums, then the n new ones, whose first has the absolute
    index `first`.  Returns a list of Python integers."""
    q, T = taps()
    nt = len(q)
    x = [int(v) for v in line]
    n = len(x) - (nt - 1)
    k0, k1 = frames_after(first), frames_after(first + n)
    if exact_python is None:
        exact_python = (k1 - k0) <= 600
    half = 1 << (T - 1)
    if exact_python:
        out = []
        for k in range(k0, k1):
            c = 2 * k - first + (nt - 1)                 # position of x[2k] in the line
            v = sum(q[j] * x[c - j] for j in range(nt))
            assert abs(v) < 1 << 59
            out.append((v + half) >> T)
        return out
    assert max(abs(v) for v in x) * sum(abs(v) for v in q) < 1 << 62          # int64 arithmetic is exact
    xa = np.array(x, dtype=np.int64)
    qa = np.array(q, dtype=np.int64)
    c0 = 2 * k0 - first + (nt - 1)
    if k1 <= k0:
        return []
    # window of frame k: x[c - nt + 1 .. c], dotted with q reversed
    win = np.lib.stride_tricks.sliding_window_view(xa, nt)[c0 - (nt - 1)::2][:k1 - k0]
    v = win @ qa[::-1]
    return [int(t) for t in ((v + half) >> T)]


def half_frames(O, X, S, first=0, hist=None, bit_depth=24, dither="X", level_db=0.0, seed=0, exact_python=None):
    """The frames and peaks of one call: X (channels, n) the new sums, hist (channels, NT - 1) the carried ones (default: zeros, the start of
    a stream).  Returns (uint8 array, float64 peaks per channel)."""
    q, _ = taps()
    X = np.asarray(X, dtype=np.int64)
    C_ = X.shape[0]
    if hist is None:
        hist = np.zeros((C_, len(q) - 1), dtype=np.int64)
    gain = math.pow(10.0, level_db / 20.0)
    k0 = frames_after(first)
    ys = []
    for c in range(C_):
        w = half_w(np.concatenate([np.asarray(hist[c], dtype=np.int64), X[c]]), first, exact_python)
        assert all(abs(t) < 1 << 33 for t in w)
        ys.append([math.ldexp(float(t), -S) for t in w])
    out = bytearray()
    for i in range(len(ys[0]) if ys else 0):
        for c in range(C_):
            out += mix_ref.emit(O, ys[c][i], c, k0 + i, bit_depth, dither.upper(), gain, seed)
    peaks = np.array([max((abs(v * gain) for v in ys[c]), default=0.0) for c in range(C_)])
    return np.frombuffer(bytes(out), dtype=np.uint8), peaks


def stream_frames(O, kw, bufs, S, **epi):
    """The whole conversion of the stream fed in the calls `bufs` by a halved engine of kw (output_rate 44100 / 48000): (bytes, peaks, sums)"""
    X = sums_at(O, kw, bufs, S)
    b, p = half_frames(O, X, S, **epi)
    return b, p, X
