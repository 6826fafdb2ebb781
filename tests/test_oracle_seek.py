"""orc_seek (oracle/d2d_oracle.c): the oracle standing at any stream position, pinned WITHOUT the engine, so that the GPU tests at frame
indices and byte positions past 2^32 (tests/test_gpu_long_streams.py) have a reference that is not a second copy of the engine's assumptions.

Each property comes from first principles:
  * low positions: seek + halo + the rest of the stream gives the rows of the uninterrupted conversion (every filter family);
  * high positions without dither: the converter is time invariant, so a context sought to a position where the output grid and the bit grid
    line up produces a fresh context's bytes, whatever the indices are;
  * high positions with dither: the requantisation is replayed in numpy from the oracle's own pre-dither samples and the generator
    rng(seed, channel, n) with the 64-bit n, sample by sample, none left out;
  * frame counts after a seek are differences of a fresh context's counts."""
import numpy as np
import pytest

from helpers import decode_pcm, pack_layout, random_bytes
from test_gpu_timeslice import CASES, NS_ALIGN

ENGINE_ONLY = ("kernel", "channel_first", "channel_count")
HALO = 4096                                  # the engine asserts preroll_bytes() <= 4096 (tests/test_gpu_timeslice.py)
PL = dict(fmt="P", endianness="L", block_size=4096)
BASES = (1 << 32, 3 << 32)


def F_of(O, kw):
    """p -> frames an uninterrupted conversion has produced after p bytes per channel (orc_max_frames of a context that is never fed)"""
    return O.Oracle(**kw).max_frames


def pos_of_frame(F, i, Mb):
    """the smallest byte position p, a multiple of Mb, with F(p) >= i (F only moves at multiples of Mb)"""
    lo, hi = 0, 1
    while F(hi * Mb) < i:
        hi *= 2
    while lo < hi:
        mid = (lo + hi) // 2
        if F(mid * Mb) >= i:
            hi = mid
        else:
            lo = mid + 1
    return lo * Mb


@pytest.mark.parametrize("cid", sorted(CASES))
def test_low_positions_seek_halo_and_the_rest_equal_the_uninterrupted_conversion(oracle_mod, cid):
    O = oracle_mod
    kw0, cuts = CASES[cid]
    kw = {k: v for k, v in dict(kw0, filter="E", seed=1000 + sorted(CASES).index(cid)).items() if k not in ENGINE_ONLY}
    Cn, fmt, blk = kw["channels"], kw["fmt"], kw["block_size"]
    if cid in NS_ALIGN:                      # noise-shaped: begin on a segment boundary, where the loop restarts whatever the halo left in it
        begin = NS_ALIGN[cid][0]
        L = begin + 6000
    else:
        begin, L = 16411, 24776              # odd, no multiple of any Mb
    q = begin - HALO
    chans = [random_bytes(L, 50 * sorted(CASES).index(cid) + c) for c in range(Cn)]
    pack = lambda a, z: pack_layout([c[a:z] for c in chans], fmt, blk)
    F = F_of(O, kw)
    if cid in NS_ALIGN:
        assert F(begin) % 8192 == 0 and F(begin) > 0

    whole = O.Oracle(**kw)
    want, fr, wy = whole.translate(pack(0, L), want_f64=True)
    fb = whole.frame_bytes
    assert fr == F(L)

    o = O.Oracle(**kw)
    o.translate(pack(0, 5000))               # a used context: the seek has to bring back every piece of a fresh one's state
    o.seek(q)
    got, gfr, gy = o.translate(pack(q, L), want_f64=True)
    drop = F(begin) - F(q)
    assert drop > 0 and gfr == F(L) - F(q)
    assert np.array_equal(got[drop * fb:gfr * fb], want[F(begin) * fb:fr * fb])
    assert gfr - drop == fr - F(begin) > 200                     # (8365 bytes: 284 frames at DSD512 -> 96 kHz, the fewest)
    for c in range(Cn):
        assert float(np.abs(gy[drop:, c]).max()) == float(np.abs(wy[F(begin):, c]).max())        # the peaks since `begin`
        assert o.peak(c) == float(np.abs(gy[:, c]).max())                                          # ... and the meter restarted at the seek
    # every frame, the halo's included, is what a context that was never fed gives from q: bit history, stage-A history, shaper errors and
    # peaks of the used context are gone
    f = O.Oracle(**kw)
    f.seek(q)
    fgot, ffr = f.translate(pack(q, L))
    assert ffr == gfr and np.array_equal(fgot, got)
    assert [f.peak(c) for c in range(Cn)] == [o.peak(c) for c in range(Cn)]
    # the halo matters: the frames right behind the seek are NOT the stream's (idle history), or this test could not tell a seek from none
    assert not np.array_equal(got[:drop * fb], want[F(q) * fb:F(begin) * fb])


# (dsd_rate, output_rate): the 44.1k family, the composed polyphase rates and the cascade
RATES = [(1, 88200), (4, 1411200), (1, 96000), (2, 384000), (4, 96000), (8, 192000)]


def aligned_position_below(O, kw, base):
    """(P, F(P), Mb): a byte position at which the output grid and the bit grid line up as they do at 0, with F(P) just below `base`"""
    o0 = O.Oracle(**kw)
    inf = o0.info()
    Mb, L = inf["M"] // 8, inf["L"]
    F = o0.max_frames
    if not L:                                # one output per Mb bytes
        P = (base - 300) * Mb
        assert F(P) == base - 300 and P % Mb == 0
        return P, F(P), Mb
    Mdn = 352800 * L // kw["output_rate"]    # output m sits at t = m Mdn on a grid of L steps per stage-A sample: y[m] reads phase t mod L at sample t div L
    assert 352800 * L == Mdn * kw["output_rate"]
    cycle = Mdn * Mb                         # bytes in which the filter runs through all its phases once: L outputs
    k = (base - 1) // L
    P = k * cycle
    assert F(cycle) == L and F(P) == k * L and F(P + cycle) - F(P) == L
    assert (F(P) * Mdn) % L == 0 and (F(P) * Mdn) // L * Mb == P          # the first output's phase is 0 and its sample is the first one behind P
    assert 0 < base - F(P) <= L
    return P, F(P), Mb


@pytest.mark.parametrize("bits", [16, 24, 32])
@pytest.mark.parametrize("base", BASES)
@pytest.mark.parametrize("rate", RATES)
def test_high_positions_without_dither_are_a_fresh_context_shifted(oracle_mod, rate, base, bits):
    O = oracle_mod
    kw = dict(dsd_rate=rate[0], output_rate=rate[1], channels=2, bit_depth=bits, dither="X", filter="E", seed=5, **PL)
    P, FP, Mb = aligned_position_below(O, kw, base)
    n1, n2 = pos_of_frame(F_of(O, kw), 700, Mb) + 3, 1001               # some 700 frames, then a ragged call
    chans = [random_bytes(n1 + n2, 7 + c) for c in range(2)]
    a, b = O.Oracle(**kw), O.Oracle(**kw)
    a.seek(P)
    crossed = 0
    for lo, hi in ((0, n1), (n1, n1 + n2)):
        buf = pack_layout([c[lo:hi] for c in chans], "P", 4096)
        ra, fa = a.translate(buf)
        rb, fb_ = b.translate(buf)
        assert fa == fb_ > 0 and np.array_equal(ra, rb)
        crossed += fa
    assert FP < base < FP + crossed                                       # the calls did run across the boundary
    assert [a.peak(c) for c in range(2)] == [b.peak(c) for c in range(2)]


def replay(O, kw, pre, first, got_bytes):
    """emit_sample in numpy: pre = the oracle's pre-dither samples (level 0 dB: they are the filter's output y), frame i has index first + i"""
    bits, dither, seed = kw["bit_depth"], kw["dither"], kw["seed"]
    Cn = pre.shape[1]
    got = decode_pcm(got_bytes, bits, Cn)
    assert got.shape == pre.shape
    checked = 0
    for c in range(Cn):
        e1 = e2 = 0.0
        for i in range(pre.shape[0]):
            n = first + i
            z = O.rng(seed, c, n)
            y = float(pre[i, c])
            if bits == 32:
                x = y * 1.0
                if dither == "F":
                    e = (int(np.float32(x).view(np.uint32)) >> 23) & 0xFF
                    expon = e - 126 if e else 0
                    t = (float(z) - 2147483647.0) * 5.5e-36
                    x = x + float(np.ldexp(t, expon + 62))
                assert np.float32(x).view(np.uint32) == got[i, c].view(np.uint32), (c, n)
                checked += 1
                continue
            x = y * 2.0 ** (bits - 1)
            d = 0.0
            if dither in "TN":
                d = float((z & 0xFFFF) + (z >> 16) + 1) * 2.0 ** -16 - 1.0
            elif dither == "R":
                d = float(2 * (z >> 16) + 1) * 2.0 ** -17 - 0.5
            w = x
            if dither == "N":
                if n % 8192 == 0:
                    e1 = e2 = 0.0
                w = x - (2.0 * e1 - e2)
            q = w + d
            r = np.floor(q + 0.5) if q >= 0.0 else np.ceil(q - 0.5)
            if dither == "N":
                e2, e1 = e1, r - w
            lim = 2.0 ** (bits - 1)
            r = min(max(r, -lim), lim - 1.0)
            assert got[i, c] == int(r), (c, n)
            checked += 1
    return checked


@pytest.mark.parametrize("base", BASES)
@pytest.mark.parametrize("dither,bits", [("T", 16), ("T", 24), ("R", 16), ("R", 24), ("F", 32), ("N", 16), ("N", 24)])
@pytest.mark.parametrize("rate", [(1, 88200), (1, 96000), (4, 96000)])
def test_high_positions_with_dither_replayed_from_the_64_bit_index(oracle_mod, rate, dither, bits, base):
    O = oracle_mod
    kw = dict(dsd_rate=rate[0], output_rate=rate[1], channels=2, bit_depth=bits, dither=dither, filter="E", seed=0x5EED0000 + bits, **PL)
    F = F_of(O, kw)
    Mb = O.Oracle(**kw).info()["M"] // 8
    P, end = pos_of_frame(F, base - 700, Mb), pos_of_frame(F, base + 700, Mb)
    assert F(P) == base - 700 and F(end) == base + 700
    chans = [random_bytes(end - P, 11 + c) for c in range(2)]
    o = O.Oracle(**kw)
    o.seek(P)                                # (the shaper starts from e1 = e2 = 0 here, as the replay does; 2^32 and 3 * 2^32 are segment starts)
    out, fr, pre = o.translate(pack_layout(chans, "P", 4096), want_f64=True)
    assert fr == 1400
    assert replay(O, kw, pre, base - 700, out[:fr * o.frame_bytes]) == 2 * 1400           # every sample, none left out
    # the generator at those indices is not the generator at their low halves: the key moves by kstep per 2^32
    words = lambda n0: [O.rng(kw["seed"], 0, n0 + n) for n in range(8)]
    assert words(base) != words(0) and words(1 << 32) != words(3 << 32)


@pytest.mark.parametrize("rate", RATES)
def test_frame_counts_after_a_seek_are_differences_of_a_fresh_contexts(oracle_mod, rate):
    O = oracle_mod
    kw = dict(dsd_rate=rate[0], output_rate=rate[1], channels=1, bit_depth=24, dither="T", filter="E", seed=1, **PL)
    F = F_of(O, kw)
    Mb = O.Oracle(**kw).info()["M"] // 8
    o = O.Oracle(**kw)
    positions = [0, 1, 4095, 16411, (1 << 29) - 1, 1 << 29, (1 << 31) + 5, 1 << 32, (1 << 32) + 12345]
    for base in BASES:
        p = pos_of_frame(F, base, Mb)
        positions += [p - 7 * Mb - 1, p - Mb, p - 1, p, p + 1, p + 33 * Mb + 3]
    for P in positions:
        o.seek(P)
        for L in (0, 1, Mb - 1, Mb, 333, 4096, 100001):
            assert o.max_frames(L) == F(P + L) - F(P), (P, L)
        buf = random_bytes(333, 3)
        _, fr = o.translate(buf)
        assert fr == F(P + 333) - F(P)
        assert o.max_frames(4096) == F(P + 333 + 4096) - F(P + 333)
