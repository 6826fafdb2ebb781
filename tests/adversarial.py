"""Bit streams that attain the worst-case sums of a tap table (a helper module like helpers.py, not a conftest).

Every matrix-core kernel is bit-exact because a partial sum stays inside a number format (mx_exact, px_exact, the
int8 kernels' limb sums, |v| < 2^31).  Sines, noise and all-ones never produce the values those claims are about: all-ones gives v = +2^S and
nothing larger.  A window of the stream whose bits follow the SIGN of a pattern P over the window's taps drives sum P_j b_j to its attainable
extreme: P = the taps themselves gives v = +-sum|q| (1.3 to 1.6 of full scale), P = one base-32 digit of 2q, one f32 part of the fp6
recombination or one base-256 limb of the int8 tables gives that partial sum's extreme.

This module reads filters/filter_tables.json ONLY -- not the filters/filter_tables.inc the engine and the oracle compile -- and restates the
decompositions in Python, so that the closed form `exact` (sum g_j s_j in Python integers) is a second reading of the tables.

A stream is a time-ordered array of bits: seeded random fill, one window every W outputs, the kinds rotating from window to window.
Coverage is a condition, not a measurement: build_* asserts that every kind has visited every output index modulo the kernel's tile T."""
import json
import math
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT_BYTES = 2 << 20                      # a stream stays under 2 MiB per channel
_TABLES = None


def tables():
    global _TABLES
    if _TABLES is None:
        with open(os.path.join(ROOT, "filters", "filter_tables.json")) as f:
            j = json.load(f)
        _TABLES = {"filters": {t["name"]: t for t in j["filters"]}, "polys": {t["name"]: t for t in j["polys"]}}
    return _TABLES


def fir_taps(name, tap_bits=24):
    """(full taps as an int64 array, scale S, decimation M): reversed(q) + q; the 32-bit grid is q32 at S + 8"""
    t = tables()["filters"][name]
    half = [int(v) for v in (t["q32"] if tap_bits == 32 else t["q"])]
    g = np.array(half[::-1] + half, dtype=np.int64)
    assert g.size == t["N"]
    return g, t["S"] + (8 if tap_bits == 32 else 0), t["M"]


def poly_taps(name):
    """(q[Lp][NP] as int64, the table's record)"""
    t = tables()["polys"][name]
    return np.array([int(v) for v in t["q"]], dtype=np.int64).reshape(t["Lp"], t["NP"]), t


def digits32(v, nd):
    """balanced base-32 digits of the integer v, least significant first: v = sum d_l 32^l, every d in [-16, 15]"""
    v = int(v)
    out = []
    for _ in range(nd):
        d = ((v + 16) & 31) - 16
        out.append(d)
        v = (v - d) // 32
    assert v == 0, "the value does not fit the digits"
    return out


def limbs256(v):
    """balanced base-256 limbs of the integer v, least significant first: every limb in [-128, 127]"""
    v = int(v)
    out = []
    for _ in range(4):
        d = ((v + 128) & 255) - 128
        out.append(d)
        v = (v - d) // 256
    assert v == 0, "the value does not fit four limbs"
    return out


def f32_parts(g, nd, m128=False):
    """the parts the fp6 kernels form in f32 from the digit sums of 2g, as per-tap integers: {name: int64 array}.
    Five digits: lo = d0 + 32 d1 + 1024 d2, hi = d3 + 32 d4 (M = 128: d0 + 32 d1 | d2 + 32 d3 + 1024 d4).
    Seven digits: lo as above, mid = d3 + 32 d4, hi = d5 + 32 d6.  Also the digits themselves, d32_l."""
    d = np.array([digits32(2 * int(q), nd) for q in g], dtype=np.int64).T          # [digit][tap]
    p = {"d32_%d" % l: d[l] for l in range(nd)}
    if nd == 7:
        assert not m128
        p["lo"], p["mid"], p["hi"] = d[0] + 32 * d[1] + 1024 * d[2], d[3] + 32 * d[4], d[5] + 32 * d[6]
    elif m128:
        p["lo"], p["hi"] = d[0] + 32 * d[1], d[2] + 32 * d[3] + 1024 * d[4]
    else:
        p["lo"], p["hi"] = d[0] + 32 * d[1] + 1024 * d[2], d[3] + 32 * d[4]
    return p


def limb_parts(g, bitpos):
    """the int8 kernels' limb sums, as per-tap integers.  A tap that meets bit position p of its stream byte is stored as the four limbs
    of q 2^(7-p) (p = 7: of -q), and the bit arrives as 2^p (p = 7: -128): build_mfma_tables / build_mfma2_tables.  Tap j's contribution to
    limb sum l is limb_l(q 2^(7-p)) 2^p, negated for p = 7.  `bitpos[j]` is p of tap j (it does not depend on the output: M is a multiple of 8)."""
    out = np.zeros((4, len(g)), dtype=np.int64)
    for j, (q, p) in enumerate(zip(g, bitpos)):
        lm = limbs256(-int(q) if p == 7 else int(q) << (7 - p))
        for l in range(4):
            out[l, j] = -128 * lm[l] if p == 7 else lm[l] << p
    return {"l256_%d" % l: out[l] for l in range(4)}


def patterns(g, grid, M=0, msb_first=False, limbs=True):
    """the patterns P of one window of taps g, in a fixed order: [(name, int64 array)].  grid: 24 or 32."""
    nd = 7 if grid == 32 else 5
    fp = f32_parts(g, nd, m128=(M == 128 and nd == 5))
    pats = [("whole", np.asarray(g, dtype=np.int64)), ("lo", fp["lo"])]
    if nd == 7:
        pats.append(("mid", fp["mid"]))
    pats.append(("hi", fp["hi"]))
    pats += [("d32_%d" % l, fp["d32_%d" % l]) for l in range(nd)]
    if limbs and grid == 24:
        n = len(g)
        t = (np.arange(n) - n) % 8                                  # time index of tap j modulo 8: ((n + 1) M - N + j) mod 8
        bitpos = 7 - t if msb_first else t
        lp = limb_parts(g, bitpos)
        pats += [("l256_%d" % l, lp["l256_%d" % l]) for l in range(4)]
    return pats


def kinds_of(pats):
    """both polarities of every pattern: [(kind name, bits of the window as uint8)].  The accumulators start from -2^S, so the two
    polarities are not mirror images of one another inside a kernel."""
    out = []
    for name, p in pats:
        out.append((name + "+", (p > 0).astype(np.uint8)))
        out.append((name + "-", (p < 0).astype(np.uint8)))
    return out


def exact_sum(g, bits):
    """sum g_j s_j with s = +1 / -1 for bit 1 / 0, as a Python int"""
    g = [int(v) for v in g]
    return sum(q if b else -q for q, b in zip(g, bits))


def _coprime_at_least(x, T):
    while math.gcd(x, T) != 1:
        x += 1
    return x


class Stream:
    """bits: the channel in time order (uint8 0 / 1); windows: [(output index, kind name, exact integer)]; S: the scale of `exact`;
    sum_abs: sum |g| of the table (of the largest phase for a polyphase table); T, K, W: tile, padded kind count, window spacing"""

    def __init__(self, bits, windows, S, sum_abs, T, K, W, kind_names):
        self.bits, self.windows, self.S, self.sum_abs, self.T, self.K, self.W, self.kind_names = bits, windows, S, sum_abs, T, K, W, kind_names
        assert bits.size % 8 == 0 and bits.size // 8 < LIMIT_BYTES, bits.size // 8
        seen = {(k, n % T) for n, k, _ in windows}
        assert len(seen) == len(kind_names) * T and {k for k, _ in seen} == set(kind_names), "a kind has not visited every residue of the tile"

    @property
    def nbytes(self):
        return self.bits.size // 8

    def packed(self, msb_first=False):
        return np.packbits(self.bits, bitorder="big" if msb_first else "little")


def _schedule(nkinds, T, wmin):
    """K >= nkinds and W >= wmin with K W coprime to T: window i sits W i outputs after the first and carries kind (i + rotate) mod K of the
    list padded cyclically to K, so kind k sits at outputs W (k + K r), r = 0 .. T - 1: every residue modulo T, since K W is a unit there."""
    return _coprime_at_least(nkinds, T), _coprime_at_least(wmin, T)


def build_fir(name, tap_bits=24, T=64, seed=0, rot=(0, 1), msb_first=False):
    """44.1k family (and stage A of the cascade): y[n] = sum_j h[j] s[(n + 1) M - N + j]; the window of output n is bits [(n + 1) M - N, (n + 1) M).
    `msb_first` only selects which bit position a tap meets for the l256 kinds (the bits returned are in time order either way)."""
    g, S, M = fir_taps(name, tap_bits)
    N = g.size
    kinds = kinds_of(patterns(g, tap_bits, M=M, msb_first=msb_first))
    exact = [exact_sum(g, b) for _, b in kinds]
    K, W = _schedule(len(kinds), T, -(-N // M))                      # W M >= N: windows do not overlap
    nwin, rotate = K * T, K * rot[0] // rot[1]                       # rot = (a, b): the kind list rotated by a / b of its length
    n0 = W                                                           # (n0 + 1) M - N >= 0
    nout = n0 + nwin * W + 3
    bits = np.random.default_rng(seed).integers(0, 2, nout * M, dtype=np.uint8)
    windows = []
    for i in range(nwin):
        n = n0 + i * W
        k = ((i + rotate) % K) % len(kinds)
        bits[(n + 1) * M - N:(n + 1) * M] = kinds[k][1]
        windows.append((n, kinds[k][0], exact[k]))
    return Stream(bits, windows, S, int(np.abs(g).sum()), T, K, W, [k for k, _ in kinds])


def build_poly(name, T=64, seed=0, rot=(0, 1)):
    """composed polyphase: output m, tt = m Mp, q = tt // Lp, rho = tt % Lp; tap j of phase rho meets bit q + D - j (d2d_poly_plain_kernel).
    The kinds are those of the output's own phase.  No limb kinds: no int8 kernel reads these tables.  With the sixteen kinds that remain, every
    table keeps full coverage (every kind at every residue modulo 5 * 32 * groups) inside the size limit (the largest, P_4_384000, is 1.1 MB),
    so no kind falls back to residues modulo 5 * groups only."""
    q2, t = poly_taps(name)
    Lp, Mp, NP, D, S = t["Lp"], t["Mp"], t["NP"], t["D"], t["S"]
    per_phase = []
    for rho in range(Lp):
        kinds = kinds_of(patterns(q2[rho], 24, limbs=False))
        per_phase.append([(kn, b, exact_sum(q2[rho], b)) for kn, b in kinds])
    nk = len(per_phase[0])
    wmin = -(-NP * Lp // Mp)                                         # floor(W Mp / Lp) >= NP: windows do not overlap
    while (wmin * Mp) // Lp < NP:
        wmin += 1
    K, W = _schedule(nk, T, wmin)
    nwin, rotate = K * T, K * rot[0] // rot[1]
    m0 = -(-(NP - D) * Lp // Mp) + 1                                 # q + D - (NP - 1) >= 0
    nout = m0 + nwin * W + 3
    nbits = ((nout * Mp // Lp + max(D, 0) + 64) + 7) // 8 * 8
    bits = np.random.default_rng(seed).integers(0, 2, nbits, dtype=np.uint8)
    windows = []
    last_top = -1
    for i in range(nwin):
        m = m0 + i * W
        q, rho = (m * Mp) // Lp, (m * Mp) % Lp
        k = ((i + rotate) % K) % nk
        kn, b, ex = per_phase[rho][k]
        top = q + D                                                  # tap 0's bit; tap j meets bit top - j
        assert top - (NP - 1) > last_top and top < nbits
        bits[top - (NP - 1):top + 1] = b[::-1]
        last_top = top
        windows.append((m, kn, ex))
    return Stream(bits, windows, S, int(np.abs(q2).sum(axis=1).max()), T, K, W, [kn for kn, _, _ in per_phase[0]])


# ---- which table a conversion runs, and the tile of the kernel that serves it in production ----
# T, outputs per tile of the production kernel for stereo frames:
#   M = 8, 16        the int8 pipelined kernel: M2_TILE = 512 (d2d_mfma.h)
#   M = 32, 64, 128  the fp6 kernel: TILE = 32 PH G with PH = 6 phases and G = mx_g(MB) = 3 / 2 / 1 groups (d2d_mx.h, d2d_mx_kernel.h): 576 / 384 / 192
#   tap_bits = 32    the fp6 kernel's seven-digit flavour: PH = 4, the same G: 384 / 256
#   polyphase        d2d_fir_px_kernel: TILE = 160 G = 5 * 32 * groups, G from D2D_PX_UNIT_LIST (d2d_px.h)
#   64               a kernel without tile structure (LUT, plain polyphase)
FIR_TILE = {8: 512, 16: 512, 32: 576, 64: 384, 128: 192}
WIDE_TILE = {32: 384, 64: 256}
POLY_GROUPS = {"P_1_96000": 3, "P_1_192000": 4, "P_1_384000": 4, "P_2_96000": 2, "P_2_192000": 3, "P_2_384000": 4, "P_4_192000": 2, "P_4_384000": 3}
# the filters that serve frames: name -> (dsd_rate, output_rate, filter letter)
FRAME_FILTERS = {
    "E_M8": (1, 352800, "E"), "E_M16": (1, 176400, "E"), "E_M32": (1, 88200, "E"), "E_M64": (2, 88200, "E"), "E_M128": (4, 88200, "E"),
    "X_M8": (1, 352800, "X"), "X_M16": (1, 176400, "X"), "X_M32": (1, 88200, "X"), "D_M8": (1, 352800, "D"),
    "C_M16": (2, 352800, "C"), "C_M32": (2, 176400, "C"), "C_M64": (2, 88200, "C"),
}
POLYS = {n: (int(n.split("_")[1]), int(n.split("_")[2])) for n in POLY_GROUPS}              # name -> (dsd_rate, output_rate)
# the two-stage cascade (no composed table at these rates): stage A's filter; A_M8 / A_M16 are behind the composed tables and no engine route reaches them
CASCADES = {"A_M32": (4, 96000), "A_M64": (8, 96000)}


def table_of(dsd_rate, output_rate, filt="E"):
    """('fir' | 'poly' | 'cascade', table name) of a conversion"""
    if output_rate % 44100 == 0:
        return "fir", "%s_M%d" % (filt, 64 * dsd_rate * 44100 // output_rate)
    name = "P_%d_%d" % (dsd_rate, output_rate)
    if name in POLY_GROUPS:
        return "poly", name
    return "cascade", "A_M%d" % (8 * dsd_rate)


def build_for(dsd_rate, output_rate, filt="E", tap_bits=24, T=None, seed=0, rot=(0, 1), msb_first=False):
    """the adversarial stream of a conversion; T defaults to the production kernel's tile; rot = (a, b) rotates the kind list by a / b of its length"""
    fam, name = table_of(dsd_rate, output_rate, filt)
    if fam == "poly":
        return build_poly(name, T=T or 160 * POLY_GROUPS[name], seed=seed, rot=rot)
    M = tables()["filters"][name]["M"]
    T = T or (WIDE_TILE[M] if tap_bits == 32 else FIR_TILE[M])
    return build_fir(name, tap_bits=tap_bits, T=T, seed=seed, rot=rot, msb_first=msb_first)
