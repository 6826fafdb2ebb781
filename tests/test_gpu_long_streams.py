"""Output indices and stream positions at and beyond 2^32, on every kernel route.

Every kernel carries code that runs only when the absolute output index crosses a multiple of 2^32 (the dither counter is
lowbias32(lo32(n) + k32 + hi32(n) * kstep): the host folds hi32 of a call's first index into the job's key, each kernel adds kstep once more
where lo32 wraps inside the call), and 64-bit arithmetic that only sees large values far into a stream (the polyphase phase, 8 * e0, n L,
n >> 13, byte positions past 2^29, 2^31 and 2^32).  d2d_seek / d2d_prime put an engine there in milliseconds; orc_seek
(tests/test_oracle_seek.py pins it without the engine) puts the oracle there.  The stream is random bytes that exist only inside the window
around the boundary.  Engine: seek -> prime the halo -> a sequence of translate calls; oracle: seek -> halo (frames discarded) -> the same calls.
Every call's frames are compared with np.array_equal, the peaks with ==, tell() after every call, and every case asserts the kernel it ran.

Call patterns around the boundary index I (2^32 or 3 * 2^32), or around the index of a byte position:
  (a) straddle: from 2501 outputs below I to 1777 above (the wrap at an odd place inside a tile, several tiles of every kernel on both sides),
      3000 more wholly above (small lo32, hi32 folded into the key), a ragged tail of 333 bytes;
  (b) touch:    a call that ends exactly at I, one that starts exactly there (lo32 == 0), one more;
  (c) above:    seek straight to I + 12345 and convert two ragged calls: hi32 in the key, no wrap in any call.
The noise shaper only starts on a segment boundary behind a seek, so its cases (and with them the fp6 kernel's scratch flavour under 'N') run
a sequence of their own from 8192 outputs below I."""
import numpy as np
import pytest

from helpers import pack_layout, random_bytes

pytestmark = pytest.mark.gpu

PL = dict(fmt="P", endianness="L", block_size=4096)
IL = dict(fmt="I", endianness="L", block_size=1)
B1, B3 = 1 << 32, 3 << 32
DBG_NO_MX, DBG_NO_PIPE, DBG_MFMA_V1 = 1 << 0, 1 << 4, 1 << 5      # dsd2dxd_amd/_capi.py (asserted against it below)

# Kernel names as d2d_kernel_name() reports what a call launched:
#   d2d_fir_mx_kernel<MB, taps, groups, epilogue kind, bytes per sample (0: integers to the scratch), channel pairs per row, digits>   (fp6)
#   d2d_fir_mfma3_kernel<MB, pairs, taps (0 = dense chain), dither kind, bytes per sample>                                             (int8 pipelined)
#   d2d_fir_mfma2_kernel<MB, pairs, channels per block, epilogue>, d2d_fir_mfma_kernel<MB>, d2d_fir_lut_kernel<MB>                     (two-group, one-group, LUT)
#   d2d_fir_px_kernel<Lp, Mp, NP, groups, kind>, d2d_poly_plain_kernel                                                                 (composed polyphase)
# The cascade's and the noise shaper's own kernels run behind the FIR kernel named here.

# route -> (parameters, the kernel every call of the case must have launched)
ROUTES = {
    # fp6 pipelined
    "fp6_m32_t24": (dict(dsd_rate=1, output_rate=88200, channels=2, bit_depth=24, dither="T", **PL), "d2d_fir_mx_kernel<4, 560, 3, 1, 3, 1, 5>"),
    "fp6_m64_r16": (dict(dsd_rate=2, output_rate=88200, channels=2, bit_depth=16, dither="R", **PL), "d2d_fir_mx_kernel<8, 1104, 2, 2, 2, 1, 5>"),
    "fp6_m128_t24": (dict(dsd_rate=4, output_rate=88200, channels=2, bit_depth=24, dither="T", **PL), "d2d_fir_mx_kernel<16, 2192, 1, 1, 3, 1, 5>"),
    "fp6_f64_level": (dict(dsd_rate=1, output_rate=88200, channels=2, bit_depth=24, dither="T", level_db=-3.0, **PL), "d2d_fir_mx_kernel<4, 560, 3, 5, 3, 1, 5>"),
    "fp6_f64_float": (dict(dsd_rate=1, output_rate=88200, channels=2, bit_depth=32, dither="F", **PL), "d2d_fir_mx_kernel<4, 560, 3, 7, 4, 1, 5>"),
    "fp6_six_channels": (dict(dsd_rate=1, output_rate=88200, channels=6, bit_depth=24, dither="T", **PL), "d2d_fir_mx_kernel<4, 560, 3, 1, 3, 3, 5>"),
    "fp6_il2": (dict(dsd_rate=1, output_rate=88200, channels=2, bit_depth=24, dither="T", **IL), "d2d_fir_mx_kernel<4, 560, 3, 1, 3, 1, 5>"),
    "fp6_taps32_one_pass": (dict(dsd_rate=1, output_rate=88200, channels=2, bit_depth=24, dither="T", tap_bits=32, **PL), "d2d_fir_mx_kernel<4, 560, 3, 5, 3, 1, 7>"),
    "fp6_taps32_two_pass_mono": (dict(dsd_rate=1, output_rate=88200, channels=1, bit_depth=24, dither="T", tap_bits=32, **PL), "d2d_fir_mfma2_kernel<4, 13, 1, 2>"),
    # int8 pipelined
    "int8_m8_t24": (dict(dsd_rate=1, output_rate=352800, channels=2, bit_depth=24, dither="T", **PL), "d2d_fir_mfma3_kernel<1, 4, 0, 1, 3>"),
    "int8_m16_r16": (dict(dsd_rate=1, output_rate=176400, channels=2, bit_depth=16, dither="R", **PL), "d2d_fir_mfma3_kernel<2, 7, 0, 2, 2>"),
    "int8_m32_no_mx": (dict(dsd_rate=1, output_rate=88200, channels=2, bit_depth=24, dither="T", debug=DBG_NO_MX, **PL), "d2d_fir_mfma3_kernel<4, 13, 0, 1, 3>"),
    # two-group kernel (three channels: a single channel is left over), one-group kernel, LUT kernel
    "two_group_3ch_t20": (dict(dsd_rate=1, output_rate=88200, channels=3, bit_depth=20, dither="T", **PL), "d2d_fir_mfma2_kernel<4, 13, 2, 0>"),
    # (the two-group kernel's own fast epilogue, with its copy of the wrap test, serves stereo 24-bit at 0 dB only: reached once the pipelined kernels are off)
    "two_group_s24_no_pipe": (dict(dsd_rate=1, output_rate=88200, channels=2, bit_depth=24, dither="T", debug=DBG_NO_PIPE, **PL), "d2d_fir_mfma2_kernel<4, 13, 2, 1>"),
    "one_group_v1": (dict(dsd_rate=1, output_rate=88200, channels=2, bit_depth=24, dither="T", debug=DBG_MFMA_V1, **PL), "d2d_fir_mfma_kernel<4>"),
    "lut_176k": (dict(dsd_rate=1, output_rate=176400, channels=2, bit_depth=24, dither="T", kernel=1, **PL), "d2d_fir_lut_kernel<2>"),
    # composed polyphase
    "px_kind1_dsd64_96k": (dict(dsd_rate=1, output_rate=96000, channels=2, bit_depth=24, dither="T", **PL), "d2d_fir_px_kernel<5, 147, 751, 3, 1>"),
    # (blocks of 1024 bytes: at 1.84 bytes per output a call of pattern (a) is under two blocks of 4096, and the kernel's fast epilogue only serves
    # tiles whose bytes lie in the call's whole blocks: with 4096 the straddling tile would go through the exact epilogue and the wrap test not run)
    "px_kind2_dsd128_384k": (dict(dsd_rate=2, output_rate=384000, channels=2, bit_depth=16, dither="R", fmt="P", endianness="L", block_size=1024), "d2d_fir_px_kernel<10, 147, 539, 4, 2>"),
    "px_kind3_dsd256_192k": (dict(dsd_rate=4, output_rate=192000, channels=2, bit_depth=32, dither="F", **PL), "d2d_fir_px_kernel<5, 294, 1541, 2, 3>"),
    "px_mono": (dict(dsd_rate=1, output_rate=96000, channels=1, bit_depth=24, dither="T", **PL), "d2d_fir_px_kernel<5, 147, 751, 3, 1>"),
    "px_il2": (dict(dsd_rate=1, output_rate=96000, channels=2, bit_depth=24, dither="T", **IL), "d2d_fir_px_kernel<5, 147, 751, 3, 1>"),
    "px_plain_192k": (dict(dsd_rate=1, output_rate=192000, channels=2, bit_depth=24, dither="T", kernel=1, **PL), "d2d_poly_plain_kernel"),
    # cascade: stage B all-integer with its inner tiles, the f64 form, config 5's shape
    "cascade_dsd256_96k": (dict(dsd_rate=4, output_rate=96000, channels=2, bit_depth=24, dither="T", **PL), "d2d_fir_mx_kernel<4, 352, 3, 0, 0, 1, 5>"),
    "cascade_f64_dsd512_96k": (dict(dsd_rate=8, output_rate=96000, channels=2, bit_depth=24, dither="T", level_db=-2.0, **PL), "d2d_fir_mx_kernel<8, 688, 2, 0, 0, 1, 5>"),
    "cascade_config5_8ch_il": (dict(dsd_rate=8, output_rate=96000, channels=8, bit_depth=24, dither="T", **IL), "d2d_fir_mx_kernel<8, 688, 2, 0, 0, 1, 5>"),
}
MONO = dict(dsd_rate=1, output_rate=88200, channels=1, bit_depth=24, dither="T", **PL)
MONO_KERNEL, PAIR_KERNEL = "d2d_fir_mfma2_kernel<4, 13, 1, 0>", "d2d_fir_mx_kernel<4, 560, 3, 1, 3, 1, 5>"
# noise shaper: the int32 recurrence, the f64 loop, the general kernel, the 48k family (index m)
NS_ROUTES = {
    "ns_s16_0db": (dict(dsd_rate=1, output_rate=88200, channels=2, bit_depth=16, dither="N", **PL), "d2d_fir_mx_kernel<4, 560, 3, 0, 0, 1, 5>"),
    "ns_s24_m2db": (dict(dsd_rate=1, output_rate=88200, channels=2, bit_depth=24, dither="N", level_db=-2.0, **PL), "d2d_fir_mx_kernel<4, 560, 3, 0, 0, 1, 5>"),
    "ns_3ch": (dict(dsd_rate=1, output_rate=88200, channels=3, bit_depth=16, dither="N", **PL), "d2d_fir_mfma2_kernel<4, 13, 2, 2>"),
    "ns_48k_dsd64_96k": (dict(dsd_rate=1, output_rate=96000, channels=2, bit_depth=24, dither="N", **PL), "d2d_fir_px_kernel<5, 147, 751, 3, 4>"),
}
ENGINE_ONLY = ("kernel", "debug")


class Case:
    """one engine, one oracle, and a random stream that exists only inside the window the case's calls cover"""

    def __init__(self, d, O, kw, seed):
        assert (d.DBG_NO_MX, d.DBG_NO_PIPE, d.DBG_MFMA_V1) == (DBG_NO_MX, DBG_NO_PIPE, DBG_MFMA_V1)
        self.kw = dict(kw, filter="E", seed=seed)
        okw = {k: v for k, v in self.kw.items() if k not in ENGINE_ONLY}
        self.e = d.Engine(**self.kw)
        self.o = O.Oracle(**okw)
        self._o0 = O.Oracle(**okw)                   # never fed, never sought: its orc_max_frames is F
        self.F = self._o0.max_frames
        self.Mb = self._o0.info()["M"] // 8
        self.C = kw["channels"]
        self.fb = self.o.frame_bytes
        assert self.e.frame_bytes == self.fb
        self.pre = self.e.preroll_bytes()
        assert 0 < self.pre <= 4096
        self.seed = seed

    def pos_of(self, i):
        """the first byte position at which an uninterrupted conversion has produced i frames (bisection on F, which moves at multiples of Mb)"""
        lo, hi = 0, 1
        while self.F(hi * self.Mb) < i:
            hi *= 2
        while lo < hi:
            mid = (lo + hi) // 2
            if self.F(mid * self.Mb) >= i:
                hi = mid
            else:
                lo = mid + 1
        return lo * self.Mb

    def open(self, begin, end):
        """the stream's bytes of [begin - preroll, end); both contexts sought to the halo's first byte and fed the halo"""
        self.w0 = begin - self.pre
        assert self.w0 > 0 and end - self.w0 < 1 << 20
        self.chans = [random_bytes(end - self.w0, 100 * self.seed + c) for c in range(self.C)]
        e, o, F = self.e, self.o, self.F
        e.seek(self.w0)
        assert e.tell() == (self.w0, F(self.w0))
        e.prime(self.pack(self.w0, begin))
        assert e.tell() == (begin, F(begin))         # (indices above 2^32 come back intact)
        assert [e.peak(c) for c in range(self.C)] == [0.0] * self.C
        o.seek(self.w0)
        o.translate(self.pack(self.w0, begin))       # the halo's frames are not the stream's: discarded
        self.peaks = [0.0] * self.C

    def pack(self, a, z):
        return pack_layout([c[a - self.w0:z - self.w0] for c in self.chans], self.kw["fmt"], self.kw["block_size"])

    def call(self, a, z, kernel):
        """one translate of bytes [a, z) on both; returns the engine's frames"""
        e, o, F = self.e, self.o, self.F
        buf = self.pack(a, z)
        got, fr = e.translate(buf)
        got = got.copy()
        want, wfr, y = o.translate(buf, want_f64=True)
        want = want[:wfr * self.fb]
        assert fr == wfr == F(z) - F(a)
        if not np.array_equal(got, want):
            k = int(np.flatnonzero(got != want)[0]) // self.fb
            raise AssertionError(f"call [{a}, {z}): first differing frame {F(a) + k} = 2^32 * {(F(a) + k) >> 32} + {(F(a) + k) & 0xFFFFFFFF} "
                                 f"(frame {k} of {fr} in the call; {int((got != want).sum())} bytes differ)")
        assert np.array_equal(got, want)
        assert e.tell() == (z, F(z))
        self.check_kernel(kernel)
        if wfr:
            self.peaks = [max(self.peaks[c], float(np.abs(y[:wfr, c]).max())) for c in range(self.C)]
        assert [e.peak(c) for c in range(self.C)] == self.peaks
        return got

    def check_kernel(self, kernel):
        assert self.e.kernel_name() == kernel, self.e.kernel_name()

    def run(self, cuts, kernels):
        self.open(cuts[0], cuts[-1])
        if not isinstance(kernels, (list, tuple)):
            kernels = [kernels] * (len(cuts) - 1)
        out = [self.call(a, z, k) for a, z, k in zip(cuts[:-1], cuts[1:], kernels)]
        assert self.e.tell() == (cuts[-1], self.F(cuts[-1]))
        return out

    def close(self):
        self.e.close()
        self.o.close()


def cuts_of(case, pattern, I):
    """the byte positions of the calls of a pattern around frame index I"""
    p = case.pos_of
    if pattern == "a":
        c2 = p(I + 1777 + 3000)
        cuts = [p(I - 2501), p(I + 1777), c2, c2 + 333]
        assert case.F(cuts[0]) < I - 2400 and I + 1777 <= case.F(cuts[1]) < I + 1780
    elif pattern == "b":
        c2 = p(I + 1300)
        cuts = [p(I - 1500), p(I), c2, c2 + 777]
        assert case.F(cuts[1]) == I                  # the first call ends, and the second starts, exactly on the boundary
    else:
        cuts = [p(I + 12345), p(I + 12345 + 1501) + 1, p(I + 12345 + 3704) + 3]
        assert case.F(cuts[0]) == I + 12345
    assert all(a < z for a, z in zip(cuts[:-1], cuts[1:]))
    return cuts


@pytest.mark.parametrize("pattern", ["a", "b", "c"])
@pytest.mark.parametrize("route", sorted(ROUTES))
def test_index_2_pow_32(engine_lib, oracle_mod, route, pattern):
    kw, kernel = ROUTES[route]
    case = Case(engine_lib, oracle_mod, kw, 3000 + sorted(ROUTES).index(route))
    case.run(cuts_of(case, pattern, B1), kernel)
    case.close()


@pytest.mark.parametrize("route", ["fp6_m32_t24", "px_kind1_dsd64_96k"])
def test_index_3_times_2_pow_32(engine_lib, oracle_mod, route):
    """the key must carry hi32 * kstep, not kstep once"""
    kw, kernel = ROUTES[route]
    case = Case(engine_lib, oracle_mod, kw, 3100 + sorted(ROUTES).index(route))
    case.run(cuts_of(case, "a", B3), kernel)
    case.close()


@pytest.mark.parametrize("pos", [1 << 29, 1 << 31, 1 << 32])
@pytest.mark.parametrize("route", ["fp6_m32_t24", "px_kind1_dsd64_96k", "cascade_dsd256_96k"])
def test_stream_position_boundaries(engine_lib, oracle_mod, route, pos):
    """bit index 2^32 of a channel, 2^31 bytes and 2^32 bytes: pattern (a) around the byte position, away from every index wrap"""
    kw, kernel = ROUTES[route]
    case = Case(engine_lib, oracle_mod, kw, 3200 + sorted(ROUTES).index(route))
    I = case.F(pos)
    assert min(abs(I - B1), I) > 1 << 20             # (the position does not coincide with 2^32 outputs at this rate)
    cuts = cuts_of(case, "a", I)
    assert cuts[0] + 2000 < pos < cuts[1] - 1000
    case.run(cuts, kernel)
    case.close()


def test_mono_pair_falls_back_on_the_wrap_and_returns_above_it(engine_lib, oracle_mod):
    """pattern (a) on a mono engine: the call that holds the wrap runs the ordinary mono kernel (the pair's second job hashes index + key with a
    key that is nout further on: one wrap test would not serve both halves), the next call, two whole blocks wholly above, is a pair again"""
    case = Case(engine_lib, oracle_mod, MONO, 3300)
    c1 = case.pos_of(B1 + 1777)
    case.run([case.pos_of(B1 - 2501), c1, c1 + 8192, c1 + 8192 + 333], [MONO_KERNEL, PAIR_KERNEL, MONO_KERNEL])
    assert MONO_KERNEL != PAIR_KERNEL
    case.close()


def test_mono_pair_up_to_the_wrap(engine_lib, oracle_mod):
    """pairs of whole blocks that end 2050 and 2 outputs below 2^32 (the last index the pair may take is 2^32 - 1), the call across, a pair above"""
    case = Case(engine_lib, oracle_mod, MONO, 3301)
    b = case.pos_of(B1 - 4098)
    assert case.F(b + 16384) == B1 - 2
    case.run([b, b + 8192, b + 16384, b + 24576, b + 32768], [PAIR_KERNEL, PAIR_KERNEL, MONO_KERNEL, PAIR_KERNEL])
    case.close()


@pytest.mark.parametrize("route", sorted(NS_ROUTES))
def test_noise_shaper_across_2_pow_32(engine_lib, oracle_mod, route):
    """from the segment start 8192 outputs below 2^32: an odd 1001 outputs, then 8192 + 3 (the groups of eight are off the grid now and the wrap
    falls inside a group), then the rest; one call over the same range gives the same frames"""
    kw, kernel = NS_ROUTES[route]
    case = Case(engine_lib, oracle_mod, kw, 3400 + sorted(NS_ROUTES).index(route))
    p = case.pos_of
    begin = p(B1 - 8192)
    assert case.F(begin) == B1 - 8192 and case.F(begin) % 8192 == 0
    cuts = [begin, p(B1 - 8192 + 1001), p(B1 + 1004), p(B1 + 3000) + 1]
    assert case.F(cuts[1]) == B1 - 8192 + 1001 and case.F(cuts[2]) == B1 + 1004
    parts = case.run(cuts, kernel)
    whole = np.concatenate(parts)
    peaks = case.peaks
    # the same range in one call, on the same engine and oracle
    case.open(cuts[0], cuts[-1])
    one = case.call(cuts[0], cuts[-1], kernel)
    assert np.array_equal(one, whole)
    assert case.peaks == peaks
    case.close()
