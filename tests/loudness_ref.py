"""An independent restatement of the loudness measurement (include/dsd2dxd_amd.h, "Loudness where the PCM is") in numpy / scipy: the
K-weighting coefficients from their closed forms, the sample conversions, cells by scipy.signal.lfilter -- from rest two sub-blocks
earlier, as the product defines them, or in one uninterrupted pass, as the standard does -- and the gating.  Nothing here calls the
library.  tests/test_loudness_cpu.py and tests/test_gpu_loudness.py hold the library to it."""
import numpy as np
from scipy.signal import lfilter

PREROLL = 2


def coefficients(rate):
    """(shelf b, shelf a, high-pass b, high-pass a): the bilinear transform of the analogue prototypes"""
    f0, G, Q = 1681.974450955533, 3.999843853973347, 0.7071752369554196
    K = np.tan(np.pi * f0 / rate)
    Vh = 10.0 ** (G / 20.0)
    Vb = Vh ** 0.4996667741545416
    a0 = 1.0 + K / Q + K * K
    sb = np.array([Vh + Vb * K / Q + K * K, 2.0 * (K * K - Vh), Vh - Vb * K / Q + K * K]) / a0
    sa = np.array([1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0])
    f0, Q = 38.13547087602444, 0.5003270373238773
    K = np.tan(np.pi * f0 / rate)
    a0 = 1.0 + K / Q + K * K
    hb = np.array([1.0, -2.0, 1.0])
    ha = np.array([1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0])
    return sb, sa, hb, ha


def ten(rate):
    """the ten doubles in d2d_loud_coefficients' order"""
    sb, sa, hb, ha = coefficients(rate)
    return np.concatenate([sb, sa[1:], hb, ha[1:]])


def sample_bytes(depth):
    return 2 if depth == 16 else 4 if depth == 32 else 3


def to_float(pcm, channels, depth):
    """packed little-endian frames (a uint8 array) -> float64 of shape (frames, channels): 16 bits v / 2^15, 20 and 24 bits the 3-byte
    container value / 2^23, 32 bits the float widened"""
    pcm = np.ascontiguousarray(pcm, dtype=np.uint8)
    if depth == 16:
        x = pcm.view("<i2").astype(np.float64) / 32768.0
    elif depth == 32:
        x = pcm.view("<f4").astype(np.float64)
    else:
        b = pcm.reshape(-1, 3).astype(np.int32)
        v = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
        x = np.where(v & 0x800000, v - (1 << 24), v).astype(np.float64) / 8388608.0
    return x.reshape(-1, channels)


def pack(x, depth):
    """integers (frames, channels) -- for 20 bits the 20-bit value, stored shifted left by 4 as the translate calls do -- or floats for depth
    32, to packed little-endian bytes"""
    if depth == 32:
        return np.ascontiguousarray(x, dtype="<f4").view(np.uint8).reshape(-1)
    v = np.ascontiguousarray(x, dtype=np.int64).reshape(-1)
    if depth == 16:
        return v.astype("<i2").view(np.uint8).reshape(-1)
    if depth == 20:
        v = v << 4
    out = np.empty((v.size, 3), dtype=np.uint8)
    out[:, 0], out[:, 1], out[:, 2] = v & 0xFF, (v >> 8) & 0xFF, (v >> 16) & 0xFF
    return out.reshape(-1)


def kweight(x, rate):
    """x (frames, channels) through both filters from rest"""
    sb, sa, hb, ha = coefficients(rate)
    return lfilter(hb, ha, lfilter(sb, sa, x, axis=0), axis=0)


def cells(x, rate, restart=True, final=True):
    """(rows, channels, 2) of (energy, peak) for the float frames x of a whole stream.  restart=True: the filter of sub-block j starts from
    rest at frame max(0, j - 2) * S, the product's definition; False: one uninterrupted pass.  final: a partial last sub-block gets a row."""
    S = rate // 10
    n, ch = x.shape
    whole = n // S
    rows = whole + (1 if final and n % S else 0)
    out = np.zeros((rows, ch, 2))
    y_all = None if restart else kweight(x, rate)
    for j in range(rows):
        lo, hi = j * S, min((j + 1) * S, n)
        if restart:
            start = max(0, j - PREROLL) * S
            y = kweight(x[start:hi], rate)[lo - start:]
        else:
            y = y_all[lo:hi]
        out[j, :, 0] = np.sum(y * y, axis=0)
        out[j, :, 1] = np.max(np.abs(x[lo:hi]), axis=0)
    return out


def default_weights(channels):
    return np.array([1.0, 1.0, 1.0, 0.0, 1.41, 1.41]) if channels == 6 else np.ones(channels)


def integrate(c, rate, whole, weights=None):
    """The gating over `whole` whole sub-block rows of cells c (a partial row behind them counts for the peak only).  Returns a dict: lufs
    (None when no block lies above -70 LUFS), peak, gain_db, blocks_total, removed_absolute, removed_relative."""
    S = rate // 10
    ch = c.shape[1]
    G = default_weights(ch) if weights is None else np.asarray(weights, dtype=np.float64)
    e = c[:whole, :, 0]
    nb = max(0, whole - 3)
    power = np.array([np.sum(G * (e[b:b + 4].sum(axis=0) / (4.0 * S))) for b in range(nb)])
    with np.errstate(divide="ignore"):
        l = -0.691 + 10.0 * np.log10(power) if nb else np.zeros(0)
    peak = float(c[:, :, 1].max()) if c.size else 0.0
    above = l > -70.0
    res = dict(lufs=None, peak=peak, gain_db=0.0, blocks_total=nb, removed_absolute=int(nb - above.sum()), removed_relative=0)
    if above.any():
        rel = -0.691 + 10.0 * np.log10(power[above].mean()) - 10.0
        keep = above & (l > rel)
        res["removed_relative"] = int(above.sum() - keep.sum())
        res["lufs"] = float(-0.691 + 10.0 * np.log10(power[keep].mean()))
        res["gain_db"] = -18.0 - res["lufs"]
    return res
