"""The reference of the channel matrix, built on the oracle and nothing of the product:

  * orc_translate_f64 at 0 dB hands back every channel's pre-dither sample y_c, which is the exact integer FIR sum x_c times 2^-S;
  * the mix is formed in Python integers: v_o = sum_c m[o][c] x_c, y_o = v_o * 2^-(S+15) (exact: |v| < 2^52);
  * from y_o on, a restatement of the oracle's emit_sample (oracle/d2d_oracle.c) with orc_rng called through ctypes on
    (seed, OUTPUT channel o, frame index).

Shared by tests/test_mix_cpu.py and tests/test_gpu_mix.py."""
import math

import numpy as np

UNITY = 32768


def exact_sums(O, kw, bufs):
    """The oracle's exact integer FIR sums of a stream fed in the calls `bufs` (each a call buffer in the context's layout).
    kw: the Oracle's conversion arguments; level, depth and dither are overridden (0 dB, float, none).
    Returns (X, S): X an int64 array (channels, frames) with y = X * 2^-S, S the smallest scale on which every sample is whole."""
    o = O.Oracle(**dict(kw, level_db=0.0, bit_depth=32, dither="X"))
    ys = []
    for b in bufs:
        _, n, f64 = o.translate(b, want_f64=True)
        ys.append(f64[:n])
    o.close()
    y = np.concatenate(ys, axis=0) if ys else np.zeros((0, kw["channels"]))
    S = 0
    while S < 48 and np.any(np.ldexp(y, S) != np.rint(np.ldexp(y, S))):
        S += 1
    assert S < 48, "the oracle's samples are not on a dyadic grid"
    X = np.ldexp(y, S).astype(np.int64)
    assert np.all(np.abs(X) < 1 << 31)
    return np.ascontiguousarray(X.T), S


def mix_values(X, S, coef):
    """y_o of every frame: (out_channels, frames) float64, exact"""
    m = np.asarray(coef, dtype=object).reshape(-1, X.shape[0])
    out = np.zeros((m.shape[0], X.shape[1]), dtype=np.float64)
    for o in range(m.shape[0]):
        v = [sum(int(m[o][c]) * int(X[c][n]) for c in range(X.shape[0])) for n in range(X.shape[1])]      # Python integers
        assert all(abs(t) < 1 << 52 for t in v)
        out[o] = [math.ldexp(float(t), -(S + 15)) for t in v]
    return out


def emit(O, y, ch, n, bits, dither, gain, seed):
    """oracle/d2d_oracle.c emit_sample for T / R / F / X: the container bytes of one sample"""
    rnd = O.rng(seed, ch, n)
    if bits == 32:
        x = y * gain
        if dither == "F":
            fb = int(np.float32(x).view(np.uint32))
            e = (fb >> 23) & 0xFF
            expon = e - 126 if e else 0
            t = (float(rnd) - 2147483647.0) * 5.5e-36
            x = x + math.ldexp(t, expon + 62)
        return np.float32(x).tobytes()
    x = y * math.ldexp(gain, bits - 1)
    d = 0.0
    if dither == "T":
        d = float((rnd & 0xFFFF) + (rnd >> 16) + 1) * 2.0 ** -16 - 1.0
    elif dither == "R":
        d = float(2 * (rnd >> 16) + 1) * 2.0 ** -17 - 0.5
    q = x + d
    r = math.floor(q + 0.5) if q >= 0.0 else math.ceil(q - 0.5)
    lim = 2.0 ** (bits - 1)
    r = max(min(r, lim - 1.0), -lim)
    iv = int(r)
    if bits == 16:
        return (iv & 0xFFFF).to_bytes(2, "little")
    if bits == 20:
        iv *= 16
    return (iv & 0xFFFFFF).to_bytes(3, "little")


def mix_frames(O, X, S, coef, bit_depth=24, dither="X", level_db=0.0, seed=0, first_index=0):
    """The frames and peaks of the mix of the sums X (channels, frames): (uint8 array, float64 peaks per output channel)"""
    y = mix_values(X, S, coef)
    gain = math.pow(10.0, level_db / 20.0)
    Co, n = y.shape
    out = bytearray()
    for i in range(n):
        for o in range(Co):
            out += emit(O, float(y[o][i]), o, first_index + i, bit_depth, dither.upper(), gain, seed)
    peaks = np.array([max((abs(float(v) * gain) for v in y[o]), default=0.0) for o in range(Co)])
    return np.frombuffer(bytes(out), dtype=np.uint8), peaks


def identity(channels):
    return [[UNITY if r == c else 0 for c in range(channels)] for r in range(channels)]
