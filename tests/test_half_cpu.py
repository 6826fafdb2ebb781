"""The 2:1 decimator behind the FIR without a GPU: the committed table's conditions, d2d_half_frames_host -- the CPU
twin of the half pass, compiled from the kernel's header -- against tests/half_ref.py, every refusal of d2d_create_half (validation comes
before any device call), the kernels half_fir_params plans, digests of the reference's bytes, and a sanitised run of tools/half_fuzz.cpp.
tests/test_gpu_half.py holds the kernel and the engine to the same reference."""
import hashlib
import json
import math
import os
import subprocess

import numpy as np
import pytest

import half_ref
from helpers import decode_pcm, pack_layout, random_bytes, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dsd2dxd_amd", "csrc")
Q, T = half_ref.taps()
NT = len(Q)
H = NT - 1
TABLE_SHA256 = "a2ac60f2360e557f560778386377b266712a0bbcac1132c7d86084bcf4163df0"
IMAX = (1 << 31) - 1


# ---- the table ----

def test_table_conditions_and_digest(engine_lib):
    assert NT % 2 == 1 and NT <= 511 and T <= 28 and Q == Q[::-1]
    assert sum(Q) == 1 << T
    assert sum(abs(v) for v in Q) < 1 << 28
    nfft = 1 << 17
    Hf = np.abs(np.fft.rfft(np.array(Q, dtype=np.float64) / float(1 << T), nfft))
    f = np.arange(Hf.size) / nfft
    ripple = float(np.max(np.abs(20 * np.log10(Hf[f <= 0.22676]))))
    stop = float(np.max(20 * np.log10(np.maximum(Hf[f >= 0.25], 1e-300))))
    print(f"pass-band deviation {ripple:.3g} dB, stop band {stop:.2f} dB")
    assert ripple <= 1e-4
    assert stop <= -126.0
    with open(half_ref.TABLE, "rb") as fh:
        assert hashlib.sha256(fh.read()).hexdigest() == TABLE_SHA256
    assert engine_lib.half_taps() == (Q, T)                                   # the library serves the committed integers


# ---- the twin against the reference ----

def _line(new, hist=None):
    """(channels, H + n) int32: the carried sums (default zeros) in front of the new ones"""
    new = np.atleast_2d(np.asarray(new, dtype=np.int64))
    hist = np.zeros((new.shape[0], H), dtype=np.int64) if hist is None else np.atleast_2d(np.asarray(hist, dtype=np.int64))
    return np.concatenate([hist, new], axis=1).astype(np.int32)


def _twin_equals_ref(d, O, new, S, first=0, hist=None, **epi):
    line = _line(new, hist)
    (got, gpk), = d.half_frames_host([line], [first], S, **epi)
    want, wpk = half_ref.half_frames(O, line[:, H:], S, first=first, hist=line[:, :H], **epi)
    assert got.size == want.size and np.array_equal(got, want), (epi, first, int(np.flatnonzero(got != want)[0]) if got.size == want.size else (got.size, want.size))
    assert np.array_equal(gpk, wpk), (epi, gpk, wpk)
    return got


@pytest.mark.parametrize("bits", [16, 20, 24, 32])
@pytest.mark.parametrize("dither", ["T", "R", "F", "X"])
def test_twin_random_int32_sums(engine_lib, oracle_mod, bits, dither):
    rng = np.random.default_rng(bits * 7 + ord(dither))
    new = rng.integers(-(1 << 31), 1 << 31, (2, 301), dtype=np.int64)
    hist = rng.integers(-(1 << 31), 1 << 31, (2, H), dtype=np.int64)
    _twin_equals_ref(engine_lib, oracle_mod, new, 30, first=(1 << 33) - 101, hist=hist, bit_depth=bits, dither=dither, seed=7)


def test_python_and_int64_forms_of_the_reference_agree():
    rng = np.random.default_rng(5)
    line = rng.integers(-(1 << 31), 1 << 31, H + 700, dtype=np.int64)
    for first in (0, 1, 12345):
        assert half_ref.half_w(line, first, exact_python=True) == half_ref.half_w(line, first, exact_python=False)


@pytest.mark.parametrize("sign", [1, -1])
def test_twin_extreme_sums_follow_the_taps_signs(engine_lib, oracle_mod, sign):
    """x[2k - j] = +-(2^31 - 1) sgn q[j]: |v| = (2^31 - 1) sum |q|, the largest the definition admits, in either sign"""
    n = 2 * NT
    new = np.zeros(n, dtype=np.int64)
    c = NT + 1                                                              # x[2k] for an even first index: frame k's window lies inside the new sums
    for j in range(NT):
        new[c - j] = sign * (IMAX if Q[j] >= 0 else -IMAX)
    w = half_ref.half_w(_line(new)[0], 0)
    v_max = IMAX * sum(abs(v) for v in Q)
    assert w[c // 2] == sign * v_max + (1 << (T - 1)) >> T and abs(w[c // 2]) > 1 << 32
    for bits, dither in ((24, "T"), (16, "R"), (32, "F"), (20, "X")):
        got = _twin_equals_ref(engine_lib, oracle_mod, np.stack([new, -new]), 30, bit_depth=bits, dither=dither, seed=9)
        if bits == 24:
            v = decode_pcm(got, 24, 2)
            assert v[c // 2, 0] == ((1 << 23) - 1 if sign > 0 else -(1 << 23)) and v[c // 2, 1] == (-(1 << 23) if sign > 0 else (1 << 23) - 1)     # clipped


@pytest.mark.parametrize("sign", [1, -1])
def test_twin_ties_round_towards_plus_infinity(engine_lib, oracle_mod, sign):
    """one impulse of +-2^(T-1): v = +-q[j] 2^(T-1) lands exactly on a tie for every odd tap, and w = ceil(v / 2^T)"""
    odd = [j for j in range(NT) if Q[j] % 2]
    assert len(odd) > 50 and any(Q[j] > 0 for j in odd) and any(Q[j] < 0 for j in odd)
    n = 3 * NT
    new = np.zeros(n, dtype=np.int64)
    at = NT + 10
    new[at] = sign << (T - 1)
    w = half_ref.half_w(_line(new)[0], 0)
    ties = 0
    for k in range(len(w)):
        j = 2 * k - at
        if 0 <= j < NT:
            v = Q[j] * int(new[at])
            if Q[j] % 2:
                assert v % (1 << T) == 1 << (T - 1) and w[k] == -((-v) // (1 << T))        # on the tie, and rounded up
                ties += 1
    assert ties > 20
    # float output without dither shows w itself (|w| < 2^24: exact in a float); S = 0 keeps y = w
    got = _twin_equals_ref(engine_lib, oracle_mod, new, 0, bit_depth=32, dither="X")
    assert [int(t) for t in decode_pcm(got, 32, 1)[:, 0]] == w
    _twin_equals_ref(engine_lib, oracle_mod, new, 28, first=1, bit_depth=24, dither="T", seed=3)       # (and at an odd first index: the other taps)


def test_twin_a_constant_comes_out_as_itself(engine_lib, oracle_mod):
    c = -123456789
    new = np.full(500, c, dtype=np.int64)
    got = _twin_equals_ref(engine_lib, oracle_mod, new, 0, first=7, hist=np.full(H, c, dtype=np.int64), bit_depth=32, dither="X")
    assert np.all(decode_pcm(got, 32, 1)[:, 0] == np.float32(c))
    assert got.size == 4 * (half_ref.frames_after(7 + 500) - half_ref.frames_after(7))


def test_twin_stream_cut_into_ragged_calls(engine_lib, oracle_mod):
    """calls of 0, 1, 2, 3, an odd count and fewer than NT - 1 sums, the history carried by hand: the bytes and peaks of one call"""
    d = engine_lib
    rng = np.random.default_rng(11)
    total = 0 + 1 + 2 + 3 + 777 + (H - 5) + 0 + 1 + 400
    X = rng.integers(-(1 << 30), 1 << 30, (2, total), dtype=np.int64)
    epi = dict(bit_depth=24, dither="T", seed=5, level_db=-1.0)
    want, wpk = half_ref.half_frames(oracle_mod, X, 29, **epi)
    (whole, pk1), = d.half_frames_host([_line(X)], [0], 29, **epi)
    assert np.array_equal(whole, want) and np.array_equal(pk1, wpk)
    full = _line(X)
    got, pk, pos = [], np.zeros(2), 0
    for n in (0, 1, 2, 3, 777, H - 5, 0, 1, 400):
        (b, p), = d.half_frames_host([np.ascontiguousarray(full[:, pos:pos + H + n])], [pos], 29, **epi)
        assert b.size == 6 * (half_ref.frames_after(pos + n) - half_ref.frames_after(pos))
        got.append(b)
        pk = np.maximum(pk, p)
        pos += n
    assert pos == total and np.array_equal(np.concatenate(got), want) and np.array_equal(pk, wpk)
    # several files in one call, one of them empty
    res = d.half_frames_host([_line(X[:, :100]), _line(np.zeros((2, 0))), _line(X[:, :333])], [0, 5, 0], 29, **epi)
    assert res[1][0].size == 0 and np.array_equal(res[0][0], want[:6 * 50]) and np.array_equal(res[2][0], want[:6 * 167])


def _tone(freq, n, fs=88200.0, amp=float(1 << 27), phase=0.3):
    return np.rint(amp * np.sin(2 * np.pi * freq / fs * np.arange(n) + phase)).astype(np.int64)


def _fit_amplitude(y, freq, fs):
    """least-squares amplitude of a sine of known frequency"""
    t = np.arange(y.size)
    A = np.stack([np.sin(2 * np.pi * freq / fs * t), np.cos(2 * np.pi * freq / fs * t)], axis=1)
    a, *_ = np.linalg.lstsq(A, y.astype(np.float64), rcond=None)
    return float(np.hypot(*a))


def test_tones_stop_band_and_pass_band(engine_lib):
    """30 kHz at 88.2 kHz lies in the stop band (<= -126 dB): at 44.1 kHz nothing of it may be left above -120 dB.  1 kHz and 20 kHz lie in
    the pass band (ripple <= 1e-4 dB; the rounding of w adds 0.5 of 2^27: 3e-8 dB): within 2e-4 dB of the input level.  Float, dither X."""
    d = engine_lib
    n = 12000
    S = 28
    amp = float(1 << 27) * 2.0 ** -S
    (b, _), = d.half_frames_host([_line(_tone(30000.0, n))], [0], S, bit_depth=32, dither="X")
    y = decode_pcm(b, 32, 1)[NT:, 0].astype(np.float64)                      # (past the start-up transient: the line begins with zeros)
    down = 20 * math.log10(max(float(np.max(np.abs(y))), 1e-300) / amp)
    print(f"30 kHz: peak of the residue {down:.2f} dB")
    assert y.size > 5000 and down <= -120.0
    for freq in (1000.0, 20000.0):
        (b, _), = d.half_frames_host([_line(_tone(freq, n))], [0], S, bit_depth=32, dither="X")
        y = decode_pcm(b, 32, 1)[NT:, 0]
        dev = 20 * math.log10(_fit_amplitude(y, freq, 44100.0) / amp)
        print(f"{freq:.0f} Hz: {dev:+.6f} dB")
        assert abs(dev) <= 2e-4


# ---- refusals, before any device call ----

def test_create_half_refusals_come_before_device_errors(engine_lib):
    d = engine_lib
    base = dict(dsd_rate=1, output_rate=44100, channels=2, fmt="P", endianness="L", bit_depth=24, dither="T")
    cases = [
        (dict(output_rate=88200), -2, "44100 or 48000"),
        (dict(output_rate=22050), -2, "44100 or 48000"),
        (dict(dsd_rate=8), -2, "DSD512"),
        (dict(dsd_rate=8, output_rate=48000), -2, "DSD512"),
        (dict(dsd_rate=4, output_rate=48000), -2, "second stage"),
        (dict(filter="S", output_rate=48000), -3, "two-stage"),
        (dict(filter="D"), -3, "dsd2pcm"),
        (dict(dither="N"), -1, "noise-shaped"),
        (dict(tap_bits=32), -1, "32-bit taps"),
        (dict(channel_first=1), -1, "channel subset"),
        (dict(channel_count=1), -1, "channel subset"),
        (dict(filter="X", dsd_rate=2), -3, "XLD"),                               # what the filter choice refuses at 88200 it refuses here
        (dict(filter="C"), -3, "Chebyshev"),
        (dict(filter="X", output_rate=48000), -3, "equiripple"),
        (dict(dither="Q"), -1, "Invalid dither type; must be T, R, F, or X"),    # d2d_create's own checks still speak
        (dict(channels=0), -1, "Invalid channel count"),
    ]
    for kw, code, frag in cases:
        with pytest.raises(d.D2DError) as ei:
            d.Engine.create_half(**dict(base, **kw))
        assert ei.value.code == code and frag in ei.value.message, (kw, ei.value.code, ei.value.message)
    with pytest.raises(d.D2DError) as ei:
        d.Engine(half=True, mix=[[16384, 16384]], **base)
    assert ei.value.code == -1 and "mix" in ei.value.message
    for rate in (44100, 48000):                                                  # and d2d_create keeps refusing the two rates
        with pytest.raises(d.D2DError) as ei:
            d.Engine(**dict(base, output_rate=rate))
        assert ei.value.code == -2 and "Invalid output rate" in ei.value.message


def test_what_create_half_admits_reaches_the_device(engine_lib):
    import torch
    d = engine_lib
    for kw in (dict(dsd_rate=1, output_rate=44100), dict(dsd_rate=4, output_rate=44100, bit_depth=32, dither="F"), dict(dsd_rate=2, output_rate=48000, channels=3),
               dict(dsd_rate=1, output_rate=44100, filter="X"), dict(dsd_rate=2, output_rate=44100, filter="C", bit_depth=16)):
        kw = dict(dict(channels=2, fmt="P", endianness="L", dither="T"), **kw)
        if torch.cuda.is_available():
            e = d.Engine.create_half(**kw)
            assert e.half_factor() == 2
            e.close()
            continue
        with pytest.raises(d.D2DError) as ei:
            d.Engine.create_half(**kw)
        assert ei.value.code == -10, ei.value.message


def test_twin_refuses_bad_calls(engine_lib):
    d = engine_lib
    x = np.zeros((2, H + 8), dtype=np.int32)
    for kw, frag in ((dict(dither="N"), "dither"), (dict(bit_depth=12), "bit depth"), (dict(capacity=4 * 6 - 1), "too small")):
        with pytest.raises(d.D2DError) as ei:
            d.half_frames_host([x], [0], 28, **kw)
        assert frag in ei.value.message


# ---- the kernels the FIR pass is planned with ----

def test_half_fir_params_plans_only_listed_kernels(tmp_path):
    exe = str(tmp_path / "half_probe")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    cmd = ["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"), "-o", exe,
           "half_probe.cpp", os.path.join(CSRC, "d2d_route.cpp"), os.path.join(CSRC, "d2d_tables.cpp")]
    r = subprocess.run(cmd, cwd=os.path.join(ROOT, "tools"), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.rstrip("\n").split("\n")
    with open(os.path.join(ROOT, "tests", "golden", "kernel_instances.json")) as f:
        listed = {(row["unit"]["pass"], row["unit"]["name"], row["unit"]["depth"], bool(row["unit"]["scratch"])) for row in json.load(f)}
    assert len(lines) == 7 * 2 * 4 * 4 * 2 * 8
    seen = set()
    for line in lines:
        own, plan, *passes = line.split("\t")
        assert passes and not passes[0].startswith("error="), line
        o, p = own.split(":"), plan.split(":")
        assert int(p[1]) == 2 * int(o[1]) and p[3][-1] == "N" and p[:1] + p[2:3] + p[4:] == o[:1] + o[2:3] + o[4:], line      # the 'N' pass of the doubled rate
        for ps in passes:
            name_pass, depth, scratch, name = ps.split(" ", 3)
            assert scratch == "1", line                                       # the sums go to the scratch
            assert (name_pass, name, int(depth), True) in listed, line
            seen.add(name)
    assert len(seen) >= 3


# ---- digests of the reference's bytes: a later change of the definition shows ----

DIGEST_CASES = {
    "dsd64_44k1_stereo_24T": (dict(dsd_rate=1, output_rate=44100, channels=2, filter="E"), dict(bit_depth=24, dither="T", seed=1)),
    "dsd128_44k1_mono_16R": (dict(dsd_rate=2, output_rate=44100, channels=1, filter="E"), dict(bit_depth=16, dither="R", seed=2)),
    "dsd256_44k1_stereo_f32F": (dict(dsd_rate=4, output_rate=44100, channels=2, filter="E"), dict(bit_depth=32, dither="F", seed=3)),
    "dsd64_48k_three_20X": (dict(dsd_rate=1, output_rate=48000, channels=3, filter="E"), dict(bit_depth=20, dither="X", seed=4)),
    "dsd64_44k1_xld_24T_minus3": (dict(dsd_rate=1, output_rate=44100, channels=2, filter="X"), dict(bit_depth=24, dither="T", seed=5, level_db=-3.0)),
}


def digest_stream(kw, nbytes=8192):
    chans = [synth("sine", nbytes, seed=1 + c, dsd_rate=kw["dsd_rate"]) if c % 2 == 0 else random_bytes(nbytes, 40 + c) for c in range(kw["channels"])]
    return pack_layout(chans, "P", 4096)


def test_reference_digests(engine_lib, oracle_mod):
    """the reference's bytes for a handful of configurations are pinned, and the twin makes the same bytes from the same sums"""
    with open(os.path.join(ROOT, "tests", "golden", "half_digests.json")) as f:
        golden = json.load(f)
    assert sorted(golden) == sorted(DIGEST_CASES)
    for name, (kw, epi) in DIGEST_CASES.items():
        kw = dict(kw, fmt="P", endianness="L", block_size=4096)
        S = half_ref.SCALE[(kw["dsd_rate"], kw["output_rate"], kw["filter"])]
        want, wpk, X = half_ref.stream_frames(oracle_mod, kw, [digest_stream(kw)], S, **epi)
        assert X.shape[1] >= 500
        assert hashlib.sha256(want.tobytes()).hexdigest() == golden[name]["sha256"] and want.size == golden[name]["bytes"], name
        (got, gpk), = engine_lib.half_frames_host([_line(X)], [0], S, **epi)
        assert np.array_equal(got, want) and np.array_equal(gpk, wpk), name


# ---- the sanitised run ----

def test_twin_sanitised(tmp_path):
    exe = str(tmp_path / "half_fuzz")
    src = [os.path.join(ROOT, "tools", "half_fuzz.cpp"), os.path.join(CSRC, "half", "d2d_half_host.cpp")]
    cmd = ["g++", "-g", "-O1", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe] + src
    r = subprocess.run(cmd, cwd=os.path.join(ROOT, "tools"), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    p = subprocess.run([exe, "1", "200"], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "fuzz ok" in p.stdout and not p.stderr, (p.stdout[-500:], p.stderr[-3000:])
