"""Every kernel route on bit streams that attain the worst-case sums (tests/adversarial.py).

The matrix-core kernels are bit-exact because partial sums stay inside a number format: f32 parts below 2^24 (mx_exact, mx_wide_exact, px_exact),
int32 limb sums and v or v + 2^S below 2^31, the all-integer requantiser's sa + 2^24 < 2^31.  Ordinary inputs (sines, noise, all-ones) stay far
from those values: all-ones gives v = +2^S and nothing larger, random bits reach a quarter of an attainable part sum.  Here every window of a
stream follows the sign of the taps, of one base-32 digit, of one f32 part or of one int8 limb, so outputs reach +-sum|q| 2^-S (1.3 to 1.6 of
full scale) and every part sum its extreme, at every output index modulo the kernel's tile, with a different kind in the other channel of a pair.
tests/test_extreme_sums_cpu.py pins the oracle on the same streams against the closed form and derives the headroom table.

Every case: engine and oracle with the same parameters, the stream in three calls (whole blocks, a ragged middle, the tail), np.array_equal on
the frames, == on every channel's peak, the launched kernel's name.
  (a) every table on its production stereo route, in four formats: float at 0 dB (nothing clips; the engine's samples are also compared with
      float32(exact 2^-S) directly, which does not involve the oracle), 24-bit TPDF just below clipping (the f64 flavour's fast path), 24-bit
      TPDF and 16-bit rectangular at 0 dB (the all-integer requantiser with |v| up to sum|q|, the redo path, both rails);
  (b) every route of tests/test_gpu_long_streams.py with the E filter, an adversarial stream in every channel.
Tables no engine route reaches: A_M8 and A_M16 (stage A at DSD64 / DSD128: those rates run the composed polyphase tables)."""
import functools

import numpy as np
import pytest

import adversarial as A
from helpers import decode_pcm, pack_layout
from test_gpu_long_streams import ENGINE_ONLY, MONO, NS_ROUTES, PAIR_KERNEL, ROUTES

pytestmark = pytest.mark.gpu

DBG_NO_INTQ, DBG_NS_GENERAL, DBG_TAPS32_2PASS = 1 << 6, 1 << 7, 1 << 16      # dsd2dxd_amd/_capi.py (asserted against it below)


@functools.lru_cache(maxsize=6)
def _stream(dsd_rate, output_rate, filt, tap_bits, T, seed, rot, msb):
    return A.build_for(dsd_rate, output_rate, filt, tap_bits=tap_bits, T=T, seed=seed, rot=rot, msb_first=msb)


def tile_of(kernel):
    """outputs per tile of a kernel, from its name (the residues modulo this are what a stream must cover)"""
    name, args = kernel.rstrip(">").split("<") if "<" in kernel else (kernel, "")
    a = [int(x) for x in args.split(",")] if args else []
    if name == "d2d_fir_mx_kernel":
        return 32 * (4 if a[6] == 7 else 6) * a[2]           # TILE = 32 PH G (d2d_mx_kernel.h), PH = 6 phases with five digits, 4 with seven
    if name == "d2d_fir_px_kernel":
        return 160 * a[3]                                    # TILE = 5 * 32 * G (d2d_px_kernel.h)
    if name in ("d2d_fir_mfma3_kernel", "d2d_fir_mfma2_kernel", "d2d_fir_mfma_kernel"):
        return 512                                           # M2_TILE (d2d_mfma.h); the one-group kernel's tile of 256 divides it
    assert name in ("d2d_fir_lut_kernel", "d2d_poly_plain_kernel"), kernel
    return 64                                                # one output per lane: no tile structure


def safe_level_db(st):
    """the largest multiple of 0.5 dB at which the table's worst output stays inside full scale: gain * sum|q| 2^-S < 1"""
    peak = st.sum_abs * 2.0 ** -st.S
    k = 0
    while 10.0 ** (-0.5 * k / 20.0) * peak >= 1.0:
        k += 1
    return -0.5 * k


def convert(d, O, kw, streams, kernel, closed_form=False, rails=False, pair_calls=False, debug=0):
    """one engine and one oracle over the streams (one per channel) in three calls; returns the engine's bytes"""
    assert (d.DBG_NO_INTQ, d.DBG_NS_GENERAL, d.DBG_TAPS32_2PASS) == (DBG_NO_INTQ, DBG_NS_GENERAL, DBG_TAPS32_2PASS)
    msb = kw["endianness"] == "M"
    C, B = kw["channels"], kw["block_size"]
    chans = [st.packed(msb) for st in streams]
    n = chans[0].size
    assert len(chans) == C and all(c.size == n for c in chans)
    if pair_calls:
        # a mono stream as a planar pair: every call splits into two equal halves of whole blocks (random fill up to the next multiple)
        pad = -n % 8192
        chans = [np.concatenate([c, np.random.default_rng(9).integers(0, 256, pad, dtype=np.uint8)]) for c in chans]
        n += pad
        cuts = [0, 8192 * (n // 8192 // 3), 8192 * (2 * (n // 8192) // 3), n]
    else:
        a = B * max(1, n // B // 3) if B > 1 else n // 3
        cuts = [0, a, 2 * a + 333, n]                        # whole blocks, a ragged middle (a short last block), the tail
    ekw = dict(kw, debug=kw.get("debug", 0) | debug)
    e = d.Engine(**ekw)
    o = O.Oracle(**{k: v for k, v in kw.items() if k not in ENGINE_ONLY})
    got, ys, names = [], [], []
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        buf = pack_layout([c[lo:hi] for c in chans], kw["fmt"], B)
        g, gf = e.translate(buf)
        w, wf, y = o.translate(buf, want_f64=True)
        assert gf == wf
        w = w[:wf * o.frame_bytes]
        if not np.array_equal(g, w):
            k = int(np.flatnonzero(g != w)[0]) // o.frame_bytes
            first = sum(x.size for x in got) // o.frame_bytes + k
            near = [(c, n_, kd) for c, st in enumerate(streams) for n_, kd, _ in st.windows if abs(n_ - first) <= 2]
            raise AssertionError(f"call [{lo}, {hi}): first differing frame {first} (index mod tile {first % streams[0].T}; windows near it: {near}); "
                                 f"{int((g != w).sum())} bytes differ; kernel {e.kernel_name()}")
        names.append(e.kernel_name())
        got.append(g.copy())
        ys.append(y[:wf])
    got = np.concatenate(got)
    peaks = [e.peak(c) for c in range(C)]
    assert peaks == [o.peak(c) for c in range(C)] == [float(np.abs(np.concatenate(ys)[:, c]).max()) for c in range(C)]
    pcm = decode_pcm(got, kw["bit_depth"], C)
    if kw["bit_depth"] == 20:
        pcm = pcm >> 4                                       # (20-bit samples ride in 24 bits)
    if closed_form:
        # float output at 0 dB without dither: the sample is (float)(v 2^-S), v the closed form; no oracle in this comparison
        for c, st in enumerate(streams):
            idx = np.array([n_ for n_, _, _ in st.windows])
            want = np.array([ex * 2.0 ** -st.S for _, _, ex in st.windows]).astype(np.float32)
            bad = np.flatnonzero(pcm[idx, c] != want)
            assert bad.size == 0, [(c, st.windows[i][:2], pcm[idx[i], c], want[i]) for i in bad[:3]]
            assert peaks[c] == st.sum_abs * 2.0 ** -st.S
    if rails:
        lim = 1 << (kw["bit_depth"] - 1)
        for c in range(C):
            assert pcm[:, c].max() == lim - 1 and pcm[:, c].min() == -lim
    e.close()
    o.close()
    print("kernels:", sorted(set(names)))
    if kernel is not None:
        assert names == [kernel] * len(names), names
    return got


# ---- (a) every table on its production stereo route ----

FORMATS = ["f32", "t24_level", "t24", "r16"]
# kernel-name arguments of a format: the fp6 kernel's (epilogue kind, bytes per sample), the same with 32-bit taps, the int8 pipelined kernel's
# (dither kind, bytes per sample), the polyphase kernel's kind
FP6_FMT = {"f32": (0, 4), "t24_level": (5, 3), "t24": (1, 3), "r16": (2, 2)}
WIDE_FMT = {"f32": (4, 4), "t24_level": (5, 3), "t24": (5, 3), "r16": (6, 2)}
TABLES_A = [("fir", n) for n in A.FRAME_FILTERS] + [("poly", n) for n in sorted(A.POLYS)] + [("cascade", n) for n in A.CASCADES]


def _conversion(fam, name):
    if fam == "fir":
        return A.FRAME_FILTERS[name]
    return (A.POLYS if fam == "poly" else A.CASCADES)[name] + ("E",)


def _format_kw(fmt, st):
    if fmt == "f32":
        return dict(bit_depth=32, dither="X")
    if fmt == "t24_level":
        level = safe_level_db(st)
        assert 10.0 ** (level / 20.0) * st.sum_abs * 2.0 ** -st.S < 1.0 <= 10.0 ** ((level + 0.5) / 20.0) * st.sum_abs * 2.0 ** -st.S
        return dict(bit_depth=24, dither="T", level_db=level)
    return dict(bit_depth=24, dither="T") if fmt == "t24" else dict(bit_depth=16, dither="R")


@pytest.mark.parametrize("fam,name,fmt", [(f, n, x) for f, n in TABLES_A for x in FORMATS])
def test_every_table_on_its_production_route(engine_lib, oracle_mod, fam, name, fmt):
    dsd_rate, out_rate, filt = _conversion(fam, name)
    streams = [_stream(dsd_rate, out_rate, filt, 24, None, 500 + c, (c, 2), False) for c in range(2)]     # channel 1: the kinds rotated by half the list
    kw = dict(dsd_rate=dsd_rate, output_rate=out_rate, channels=2, fmt="P", endianness="L", block_size=4096, filter=filt, seed=21, **_format_kw(fmt, streams[0]))
    kernel = KERNELS_A.get((name, fmt))
    got = convert(engine_lib, oracle_mod, kw, streams, kernel, closed_form=fmt == "f32" and fam != "cascade",
                  # (the cascade's output is stage B's answer to a one-sample spike of +-sum|q_A|: far from the rails, and no closed form of one table)
                  rails=fmt in ("t24", "r16") and fam != "cascade")
    assert got.size and kernel is not None
    assert tile_of(kernel) == streams[0].T or fam == "cascade"


def _kernels_a():
    """the kernel every call of a case of (a) must have launched"""
    k = {}
    for name in A.FRAME_FILTERS:
        t = A.tables()["filters"][name]
        M, N = t["M"], t["N"]
        for fmt in FORMATS:
            if M >= 32:
                k[name, fmt] = "d2d_fir_mx_kernel<%d, %d, %d, %d, %d, 1, 5>" % ((M // 8, N, {32: 3, 64: 2, 128: 1}[M]) + FP6_FMT[fmt])
            else:
                k[name, fmt] = "d2d_fir_mfma3_kernel<%d, %d, 0, %d, %d>" % ((M // 8, (N + 7 * M + 24 + 63) // 64) + FP6_FMT[fmt])
    for name, G in A.POLY_GROUPS.items():
        t = A.tables()["polys"][name]
        for fmt, kind in zip(FORMATS, (3, 3, 1, 2)):                  # kind 3: the f64 flavour (float frames, another level), 1 / 2: 24-bit TPDF / 16-bit rectangular at 0 dB
            k[name, fmt] = "d2d_fir_px_kernel<%d, %d, %d, %d, %d>" % (t["Lp"], t["Mp"], t["NP"], G, kind)
    for name in A.CASCADES:
        t = A.tables()["filters"][name]
        for fmt in FORMATS:
            k[name, fmt] = "d2d_fir_mx_kernel<%d, %d, %d, 0, 0, 1, 5>" % (t["M"] // 8, t["N"], {32: 3, 64: 2}[t["M"]])        # stage A: the integers to the scratch
    return k


KERNELS_A = _kernels_a()


@pytest.mark.parametrize("name,two_pass,fmt", [(n, False, x) for n in ("E_M32", "E_M64") for x in FORMATS] + [("E_M32", True, x) for x in FORMATS])
def test_32_bit_taps(engine_lib, oracle_mod, name, two_pass, fmt):
    """tap_bits = 32: the one-pass route (seven digits, three f32 parts: the q32 kinds with `mid`), and the two scratch passes + combining pass"""
    dsd_rate, out_rate, filt = A.FRAME_FILTERS[name]
    M = A.tables()["filters"][name]["M"]
    streams = [_stream(dsd_rate, out_rate, filt, 32, A.WIDE_TILE[M], 600 + c, (c, 2), False) for c in range(2)]
    assert "mid+" in streams[0].kind_names and "d32_6-" in streams[0].kind_names
    kw = dict(dsd_rate=dsd_rate, output_rate=out_rate, channels=2, fmt="P", endianness="L", block_size=4096, filter=filt, seed=22, tap_bits=32,
              **_format_kw(fmt, streams[0]))
    if two_pass:
        kernel = TWO_PASS_KERNEL
        kw["debug"] = DBG_TAPS32_2PASS
    else:
        kernel = "d2d_fir_mx_kernel<%d, %d, %d, %d, %d, 1, 7>" % ((M // 8, 2 * len(A.tables()["filters"][name]["q"]), {32: 3, 64: 2}[M]) + WIDE_FMT[fmt])
        assert tile_of(kernel) == streams[0].T
    convert(engine_lib, oracle_mod, kw, streams, kernel, closed_form=fmt == "f32", rails=fmt in ("t24", "r16"))


TWO_PASS_KERNEL = "d2d_fir_mx_kernel<4, 560, 3, 0, 0, 1, 5>"       # both passes write integers to the scratch; d2d_fine_combine_kernel runs behind them


# ---- (b) every route with the E filter ----

def _route_streams(kw, kernel, seed):
    C = kw["channels"]
    T = tile_of(kernel)
    return [_stream(kw["dsd_rate"], kw["output_rate"], "E", kw.get("tap_bits", 24) or 24, T, seed + c, (c, C), kw["endianness"] == "M") for c in range(C)]


@pytest.mark.parametrize("route", sorted(ROUTES))
def test_every_route(engine_lib, oracle_mod, route):
    kw, kernel = ROUTES[route]
    kw = dict(kw, filter="E", seed=23)
    streams = _route_streams(kw, kernel, 700)
    fam = A.table_of(kw["dsd_rate"], kw["output_rate"])[0]
    convert(engine_lib, oracle_mod, kw, streams, kernel,
            closed_form=fam != "cascade" and kw["bit_depth"] == 32 and kw["dither"] == "X" and not kw.get("level_db"),
            rails=fam != "cascade" and kw["bit_depth"] != 32 and not kw.get("level_db"))


def test_mono_stream_as_a_planar_pair(engine_lib, oracle_mod):
    """calls that split into equal halves: the two halves run side by side as the channels of a pair, each with its own windows"""
    kw = dict(MONO, filter="E", seed=24)
    convert(engine_lib, oracle_mod, kw, _route_streams(kw, PAIR_KERNEL, 800), PAIR_KERNEL, rails=True, pair_calls=True)


@pytest.mark.parametrize("route", sorted(NS_ROUTES))
def test_noise_shaper_routes(engine_lib, oracle_mod, route):
    """the noise shaper's recurrence on |v| up to sum|q|: the production route, the same without the all-integer requantiser (DBG_NO_INTQ) and the
    general kernel (DBG_NS_GENERAL) produce identical bytes (each is compared with the oracle, so with one another).  The flags select among the
    noise shaper's own kernels, which run behind the FIR kernel: the name reported is the FIR kernel's and stays the same."""
    kw, kernel = NS_ROUTES[route]
    kw = dict(kw, filter="E", seed=25)
    streams = _route_streams(kw, kernel, 900)
    base = convert(engine_lib, oracle_mod, kw, streams, kernel)
    for flag in (DBG_NO_INTQ, DBG_NS_GENERAL):
        other = convert(engine_lib, oracle_mod, kw, streams, kernel, debug=flag)
        assert np.array_equal(other, base), flag
