"""An independent restatement of the true-peak measurement (include/dsd2dxd_amd.h, "Loudness where the PCM is"), written from its
definition and not from csrc/loud/true_peak.h: four phases of twelve integer taps over 8192, y_p(n) = sum_k C[p][k] x(n - k) with zeros
before frame 0, the value |y| / 8192, a cell the largest value over the sub-block's frames and the four phases; the outputs behind the
last frame are dropped.  Integer depths: int64 sums, scaled by exact powers of two -- no rounding anywhere.  Float: an explicit f64 loop
in tap order.  Nothing here calls the library.  tests/test_true_peak_cpu.py and tests/test_gpu_true_peak.py hold the library to it."""
import numpy as np

from loudness_ref import pack, sample_bytes, to_float  # noqa: F401  (the sample layouts are the loudness calls')

PHASE0 = [14, 90, -161, 272, -487, 1125, 7964, -838, 390, -218, 122, -68]
PHASE1 = [-239, 240, -424, 730, -1364, 3810, 6388, -1641, 832, -477, 271, -155]
COEF = np.array([PHASE0, PHASE1, PHASE1[::-1], PHASE0[::-1]], dtype=np.int64)
TAPS = 12


def integers(pcm, channels, depth):
    """packed little-endian frames -> (int64 of shape (frames, channels), log2 of the full scale): 16 bits the value over 2^15, 20 and
    24 bits the 3-byte container value over 2^23"""
    pcm = np.ascontiguousarray(pcm, dtype=np.uint8)
    if depth == 16:
        return pcm.view("<i2").astype(np.int64).reshape(-1, channels), 15
    b = pcm.reshape(-1, 3).astype(np.int64)
    v = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
    return np.where(v & 0x800000, v - (1 << 24), v).reshape(-1, channels), 23


def outputs(pcm, channels, depth):
    """|y_p(n)| / 8192 for every frame, channel and phase: float64 of shape (frames, channels, 4), exact for integer depths"""
    if depth == 32:
        x = np.ascontiguousarray(pcm, dtype=np.uint8).view("<f4").astype(np.float64).reshape(-1, channels)
        frames = x.shape[0]
        xz = np.concatenate([np.zeros((TAPS - 1, channels)), x])
        y = np.zeros((frames, channels, 4))
        for p in range(4):
            acc = np.zeros((frames, channels))                           # from 0.0, in the order k = 0, 1, .. 11: one rounded addition each
            for k in range(TAPS):
                acc = acc + float(COEF[p, k]) * xz[TAPS - 1 - k:TAPS - 1 - k + frames]      # (the product is exact)
            y[:, :, p] = acc
        return np.abs(y) * 2.0 ** -13
    v, scale = integers(pcm, channels, depth)
    frames = v.shape[0]
    vz = np.concatenate([np.zeros((TAPS - 1, channels), dtype=np.int64), v])
    y = np.zeros((frames, channels, 4), dtype=np.int64)
    for p in range(4):
        for k in range(TAPS):
            y[:, :, p] += COEF[p, k] * vz[TAPS - 1 - k:TAPS - 1 - k + frames]
    assert np.max(np.abs(y), initial=0) < 2 ** 52
    return np.abs(y).astype(np.float64) * 2.0 ** -(13 + scale)          # (under 2^53: the conversion and the scaling are exact)


def cells(pcm, channels, depth, rate, final=True):
    """the true-peak doubles of a whole stream: float64 of shape (rows, channels); a partial last row when `final`"""
    S = rate // 10
    y = outputs(pcm, channels, depth).max(axis=2)
    frames = y.shape[0]
    rows = frames // S + (1 if final and frames % S else 0)
    return np.array([y[r * S:min((r + 1) * S, frames)].max(axis=0) for r in range(rows)]).reshape(rows, channels)


def sample_peak(pcm, channels, depth):
    x = to_float(pcm, channels, depth)
    return float(np.max(np.abs(x))) if x.size else 0.0
