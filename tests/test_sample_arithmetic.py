"""The arithmetic contract of DESIGN section 2 as dsd2dxd_amd/csrc/d2d_sample.h states it once for every kernel, run on the host:
tools/sample_probe.cpp includes the header and is compiled with the flags the contract assumes (one IEEE operation per written one)."""
import ctypes
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M32 = 0xFFFFFFFF


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("sample_probe") / "sample_probe")
    cmd = ["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-o", exe, "sample_probe.cpp"]
    r = subprocess.run(cmd, cwd=os.path.join(ROOT, "tools"), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]

    def run(*args):
        p = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, (args, p.stdout[-500:], p.stderr[-500:])
        return p.stdout
    return run


def _counts(out):
    """('cases N mismatches M' on the last line) -> (N, M)"""
    w = out.strip().split("\n")[-1].split()
    assert w[0] == "cases" and w[2] == "mismatches", out[-500:]
    return int(w[1]), int(w[3])


@pytest.mark.parametrize("seed", [0, 0x1234_5678_9ABC_DEF1])
@pytest.mark.parametrize("channel", [0, 1, 5])
def test_dither_word_is_the_oracles_generator_across_a_2_32_boundary(probe, oracle_mod, seed, channel):
    """key, kstep and lo0 as the engine derives them for a call whose first index is i0 (d2d_engine.cpp: enqueue_jobs); the call's
    indices run across a multiple of 2^32, where lo32 wraps and kstep is due once more.  The second call starts above 2^32, so that
    the high half the host folds into the key is not zero."""
    L = oracle_mod.lib()
    L.orc_rng_key.argtypes = [ctypes.c_uint64, ctypes.c_uint32]
    L.orc_rng_key.restype = ctypes.c_uint64
    k = L.orc_rng_key(seed, channel)
    for i0 in ((1 << 32) - 600, (3 << 32) - 600):
        kstep = (k & M32) | 1
        key = ((k >> 32) + (i0 >> 32) * kstep) & M32
        lo0 = i0 & M32
        got = [int(x) for x in probe("rng", key, kstep, lo0, lo0, 1201).split()]
        want = [oracle_mod.rng(seed, channel, i0 + i) for i in range(1201)]
        assert got == want


@pytest.mark.parametrize("bits", [16, 24])
@pytest.mark.parametrize("F", [1, 7, 8, 15, 16])
@pytest.mark.parametrize("kind", [0, 1, 2], ids=["none", "triangular", "rectangular"])
def test_requant_int_equals_the_f64_definition(probe, kind, F, bits):
    """requant_int<KIND>(v, F, z) against round_clip(v * 2^-F + dither_f64<KIND>(dither_term<KIND>(z)), 2^(bits-1)), x formed exactly.
    The probe's v: 10^5 random ones (half anywhere in int32, half within 1.25 times the depth's range), every multiple of 2^(F-1)
    (the exact ties) near zero and both rails and 20 000 random ones, every v within 3 LSB of both rails, 0, +-1 and the ends of
    int32; v is an int32 as in the kernels, so where bits - 1 + F > 31 a rail lies outside it and the ends of int32 stand in.  Each
    v with a random hash word and with the words 0 and 2^32 - 1 (the ends of the dither's range).  Nothing is excluded."""
    cases, bad = _counts(probe("requant", kind, F, bits, 1000 * kind + 10 * F + bits, 100000))
    assert cases >= 100000 and bad == 0


def test_round_clip_and_dither_float_equal_the_first_epilogue(probe):
    """round_clip(y * scale + dither) and dither_float(y * gain) against quantise_int / quantise_f32 as d2d_device.h stated them before
    the pieces were shared (the probe keeps that text): 10^4 y (+-0, subnormal floats, the clip and the ties next to it, random ones
    down to 2^-160), three levels, 16 / 20 / 24 bits and float, no / triangular / rectangular dither: equal bit for bit."""
    cases, bad = _counts(probe("quant", 3, 10000))
    assert cases >= 10000 and bad == 0
