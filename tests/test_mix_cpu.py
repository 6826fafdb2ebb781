"""The channel matrix without a GPU: the preset table, every refusal and bound of d2d_create_mix (validation comes
before any device call), d2d_mix_frames_host -- the CPU twin of the mix pass, compiled from the kernel's header -- against tests/mix_ref.py,
and a sanitised run of tools/mix_fuzz.cpp.  tests/test_gpu_mix.py holds the kernel to the same reference."""
import os
import subprocess

import numpy as np
import pytest

import adversarial
import mix_ref
from helpers import pack_layout, random_bytes, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dsd2dxd_amd", "csrc")
U = mix_ref.UNITY


# ---- the presets ----

PRESETS = {
    # layout name: (channels, Lo, Ro)
    "5_1": (6, [13573, 0, 9597, 0, 9597, 0], [0, 13573, 9597, 0, 0, 9597]),
    "5_0": (5, [13573, 0, 9597, 9597, 0], [0, 13573, 9597, 0, 9597]),
    "QUAD": (4, [19195, 0, 13573, 0], [0, 19195, 0, 13573]),
    "LRC": (3, [19195, 0, 13573], [0, 19195, 13573]),
    "LRC_LFE": (4, [19195, 0, 13573, 0], [0, 19195, 13573, 0]),
}


def test_preset_table(engine_lib):
    d = engine_lib
    for name, (ch, lo, ro) in PRESETS.items():
        layout = getattr(d, "MIX_LAYOUT_" + name)
        assert d.mix_preset(ch, 2, layout) == [lo, ro], name
        assert d.mix_preset(ch, 1, layout) == [[(a + b) // 2 for a, b in zip(lo, ro)]], name
        assert sum(lo) <= U and sum(ro) <= U and min(lo + ro) >= 0
    assert PRESETS["5_0"][1] == [v for i, v in enumerate(PRESETS["5_1"][1]) if i != 3]          # the 5.1 rows without the LFE column
    assert PRESETS["5_0"][2] == [v for i, v in enumerate(PRESETS["5_1"][2]) if i != 3]
    assert d.mix_preset(2, 1, d.MIX_LAYOUT_STEREO) == [[16384, 16384]]
    # by channel count: 2 stereo, 3 L R C, 4 quad, 5 5.0, 6 5.1
    for ch, name in ((3, "LRC"), (4, "QUAD"), (5, "5_0"), (6, "5_1")):
        assert d.mix_preset(ch, 2) == [PRESETS[name][1], PRESETS[name][2]]
    assert d.mix_preset(2, 1) == [[16384, 16384]]
    for args, frag in (((2, 2), "stereo already"), ((7, 2), "no preset"), ((1, 1), "no preset"), ((6, 3), "target"), ((6, 0), "target"),
                       ((5, 2, d.MIX_LAYOUT_5_1), "this many channels"), ((6, 2, 99), "no preset")):
        with pytest.raises(d.D2DError) as ei:
            d.mix_preset(*args)
        assert ei.value.code == -1 and frag in ei.value.message, args


# ---- refusals and bounds, before any device call ----

def test_create_mix_refusals_come_before_device_errors(engine_lib):
    d = engine_lib
    base = dict(dsd_rate=1, output_rate=88200, channels=3, fmt="P", endianness="L", bit_depth=24, dither="T")
    ident = mix_ref.identity(3)
    cases = [
        (dict(), [[U, 0, 0]] * 4, -1, "out_channels"),                                     # Co > C
        (dict(), np.zeros((0, 3)), -1, "out_channels"),                                    # Co = 0
        (dict(), [[(1 << 17) + 1, 0, 0]], -1, "above 4.0"),
        (dict(), [[-(1 << 17) - 1, 0, 0]], -1, "above 4.0"),
        (dict(channels=17), [[1 << 17] * 16 + [1]], -1, "64.0"),                           # a row's sum of |m| = 2^21 + 1
        (dict(dither="N"), ident, -1, "noise-shaped"),
        (dict(tap_bits=32), ident, -1, "32-bit taps"),
        (dict(channel_first=1), ident, -1, "channel subset"),
        (dict(channel_count=2), ident, -1, "channel subset"),
        (dict(dsd_rate=4, output_rate=96000), ident, -3, "second stage"),                  # DSD256 -> 96 kHz
        (dict(dsd_rate=8, output_rate=96000), ident, -3, "second stage"),                  # DSD512 -> 48 kHz multiples
        (dict(output_rate=96000, filter="S"), ident, -3, "second stage"),                  # filter 'S'
        (dict(dither="Q"), ident, -1, "Invalid dither type; must be T, R, F, or X"),       # d2d_create's own checks still speak
        (dict(output_rate=44100), ident, -2, "Invalid output rate"),
    ]
    for kw, mix, code, frag in cases:
        with pytest.raises(d.D2DError) as ei:
            d.Engine(mix=mix, **dict(base, **kw))
        assert ei.value.code == code and frag in ei.value.message, (kw, ei.value.message)
    import ctypes as C
    p = d._capi.make_params(**base)
    m, keep = d._capi._mix_struct(ident, 3)
    h = C.c_void_p()
    m.struct_size = 8
    assert d.lib().d2d_create_mix(C.byref(p), C.byref(m), 1, C.byref(h)) == -1 and b"struct_size" in d.lib().d2d_create_error()
    assert C.sizeof(d.Mix) == 16


def test_what_passes_the_bounds_reaches_the_device(engine_lib):
    """at the bounds exactly, a zero row, 96 kHz on the composed tables, stereo to mono in float: validation passes.  Without a GPU the next
    error is the device's; with one the engine exists, reports its mix, and is closed again"""
    import torch
    d = engine_lib
    for kw, mix in ((dict(channels=16), [[1 << 17] * 16, [-(1 << 17)] * 16, [0] * 16]), (dict(channels=6, output_rate=96000), d.mix_preset(6, 2)),
                    (dict(channels=2, bit_depth=32, dither="F", level_db=-3.0), [[16384, 16384]])):
        kw = dict(dict(dsd_rate=1, output_rate=88200, fmt="P", endianness="L"), **kw)
        if torch.cuda.is_available():
            e = d.Engine(mix=mix, **kw)
            assert e.get_mix() == [list(r) for r in mix] and e.out_channels == len(mix)
            e.close()
            continue
        with pytest.raises(d.D2DError) as ei:
            d.Engine(mix=mix, **kw)
        assert ei.value.code == -10, ei.value.message


# ---- the DFF channel ids and the DSF channel type as layouts (the file-level C ABI; a dry run, no device) ----

def _dff(path, ids, nbytes=64):
    """a DSDIFF file whose CHNL chunk names `ids`, with a few bytes of idle pattern as audio"""
    import struct
    C_ = len(ids)
    data = bytes([0x69]) * (nbytes * C_)
    chnl = struct.pack(">H", C_) + b"".join(ids)
    cmpr = b"DSD " + bytes([14]) + b"not compressed" + b"\x00"
    prop = b"SND " + b"FS  " + struct.pack(">QI", 4, 2822400) + b"CHNL" + struct.pack(">Q", len(chnl)) + chnl + b"CMPR" + struct.pack(">Q", len(cmpr)) + cmpr
    body = b"DSD " + b"FVER" + struct.pack(">QI", 4, 0x01050000) + b"PROP" + struct.pack(">Q", len(prop)) + prop + b"DSD " + struct.pack(">Q", len(data)) + data
    with open(path, "wb") as f:
        f.write(b"FRM8" + struct.pack(">Q", len(body)) + body)


def _downmix_of_container(d, path, target=2):
    """(return code of d2dh_set_downmix, message) on a converter made by d2dh_from_container"""
    import ctypes as C
    L = C.CDLL(d.library_path())
    L.d2dh_last_error.restype = C.c_char_p
    h = C.c_void_p()
    rc = L.d2dh_from_container(C.c_uint32(24), C.c_uint32(ord("F")), C.c_double(0.0), C.c_uint32(88200), None, C.c_uint32(ord("T")), C.c_uint32(ord("E")),
                               C.c_int(0), b".", str(path).encode(), C.byref(h))
    assert rc == 0 and h.value, L.d2dh_last_error()
    rc = L.d2dh_set_downmix(h, C.c_uint32(target))
    msg = L.d2dh_last_error().decode()
    L.d2dh_free(h)
    return rc, msg


def test_container_layouts_choose_or_refuse_a_preset(engine_lib, tmp_path):
    d = engine_lib
    d.lib()
    S, R, M, N, Cc, LFE, LS, RS = b"SLFT", b"SRGT", b"MLFT", b"MRGT", b"C   ", b"LFE ", b"LS  ", b"RS  "
    served = {"51": [M, N, Cc, LFE, LS, RS], "51s": [S, R, Cc, LFE, LS, RS], "50": [M, N, Cc, LS, RS], "quad": [S, R, LS, RS], "lrc": [S, R, Cc],
              "lrclfe": [S, R, Cc, LFE]}
    for name, ids in served.items():
        _dff(tmp_path / (name + ".dff"), ids)
        assert _downmix_of_container(d, tmp_path / (name + ".dff")) == (0, ""), name
        assert _downmix_of_container(d, tmp_path / (name + ".dff"), 1) == (0, ""), name
    refused = {"swapped": [S, R, LS, RS, Cc, LFE], "numbered": [b"C000", b"C001", b"C002", b"C003", b"C004", b"C005"], "five_odd": [S, R, Cc, LFE, LS],
               "mono": [Cc]}
    for name, ids in refused.items():
        _dff(tmp_path / (name + ".dff"), ids)
        rc, msg = _downmix_of_container(d, tmp_path / (name + ".dff"))
        assert rc == -1 and "no preset serves" in msg and name + ".dff" in msg, (name, msg)
    _dff(tmp_path / "st.dff", [S, R])
    assert _downmix_of_container(d, tmp_path / "st.dff", 1) == (0, "")
    rc, msg = _downmix_of_container(d, tmp_path / "st.dff", 2)
    assert rc == -1 and "stereo already" in msg
    # DSF: the fmt chunk's channel type
    from helpers import write_dsf
    for ch, ctype, ok in ((6, 7, True), (5, 6, True), (4, 4, True), (4, 5, True), (3, 3, True), (6, 1, False), (6, 6, False), (6, 9, False)):
        p = str(tmp_path / f"c{ch}_t{ctype}.dsf")
        write_dsf(p, [np.full(4096, 0x69, dtype=np.uint8)] * ch)
        with open(p, "r+b") as f:
            f.seek(28 + 20)
            f.write(int(ctype).to_bytes(4, "little"))
        rc, msg = _downmix_of_container(d, p)
        assert (rc == 0) == ok and (ok or "downmix" in msg.lower()), (ch, ctype, msg)


# ---- the twin against the reference ----

KW = dict(dsd_rate=1, output_rate=88200, channels=3, fmt="P", endianness="L", block_size=4096, filter="E")
NB = 4096


@pytest.fixture(scope="module")
def sums3(oracle_mod):
    chans = [synth("sine", NB, seed=1), synth("pink", NB, seed=2, amp=0.3), random_bytes(NB, 3)]
    X, S = mix_ref.exact_sums(oracle_mod, KW, [pack_layout(chans, "P", 4096)])
    assert X.shape == (3, NB * 8 // 32)
    return X, S


def _twin_equals_ref(d, O, X, S, coef, **epi):
    got, gpk = d.mix_frames_host(X.astype(np.int32), S, coef, **epi)
    want, wpk = mix_ref.mix_frames(O, X, S, coef, **epi)
    assert np.array_equal(got, want), (coef, epi, int(np.flatnonzero(got != want)[0]))
    assert np.array_equal(gpk, wpk), (coef, epi)
    return got


@pytest.mark.parametrize("bits", [16, 20, 24, 32])
@pytest.mark.parametrize("dither", ["T", "R", "F", "X"])
def test_twin_every_dither_and_depth(engine_lib, oracle_mod, sums3, bits, dither):
    X, S = sums3
    coef = [[19195, 0, 13573], [-9597, 23170, 40000]]
    _twin_equals_ref(engine_lib, oracle_mod, X, S, coef, bit_depth=bits, dither=dither, seed=7, first_index=(1 << 32) - 100)


@pytest.mark.parametrize("level", [-3.0, 3.0])
def test_twin_levels(engine_lib, oracle_mod, sums3, level):
    X, S = sums3
    for bits, dither in ((24, "T"), (32, "F"), (16, "R")):
        _twin_equals_ref(engine_lib, oracle_mod, X, S, [[13573, 9597, 9597], [0, 0, U]], bit_depth=bits, dither=dither, level_db=level, seed=3)


def test_twin_identity_and_permutation_are_the_oracles_own_frames(engine_lib, oracle_mod, sums3):
    """32768 I gives the plain conversion's bytes: the reference here is the oracle's own translate, not mix_ref"""
    X, S = sums3
    chans = [synth("sine", NB, seed=1), synth("pink", NB, seed=2, amp=0.3), random_bytes(NB, 3)]
    buf = pack_layout(chans, "P", 4096)
    for bits, dither, level in ((24, "T", 0.0), (16, "R", -3.0), (32, "F", -3.0), (20, "X", 0.0)):
        o = oracle_mod.Oracle(**dict(KW, bit_depth=bits, dither=dither, level_db=level, seed=11))
        want, n = o.translate(buf)
        got = _twin_equals_ref(engine_lib, oracle_mod, X, S, mix_ref.identity(3), bit_depth=bits, dither=dither, level_db=level, seed=11)
        assert np.array_equal(got, want[:got.size]) and got.size == n * o.frame_bytes
        assert [o.peak(c) for c in range(3)] == list(engine_lib.mix_frames_host(X.astype(np.int32), S, mix_ref.identity(3), level_db=level)[1])
    # a signed permutation: output o is +- input p[o], dithered as OUTPUT channel o
    _twin_equals_ref(engine_lib, oracle_mod, X, S, [[0, 0, -U], [U, 0, 0], [0, -U, 0]], bit_depth=24, dither="T", seed=5)
    _twin_equals_ref(engine_lib, oracle_mod, X, S, [[0, U, 0], [0, 0, 0]], bit_depth=16, dither="T", seed=5)          # and a zero row


@pytest.fixture(scope="module")
def worst16(oracle_mod):
    """sixteen channels of the stream whose windows attain the table's extreme sums (tests/adversarial.py), every channel the same bits"""
    st = adversarial.build_for(1, 88200, T=64)
    one = st.packed()
    kw = dict(KW, channels=16)
    X, S = mix_ref.exact_sums(oracle_mod, kw, [pack_layout([one] * 16, "P", 4096)])
    # (exact_sums finds the smallest grid: every sum of a table has the parity of sum q = 2^S, so it is one bit coarser than the table's)
    assert S <= st.S and int(np.abs(X).max()) << (st.S - S) == st.sum_abs   # the extreme is attained
    return X, S, one


SATURATING = [[1 << 17] * 16, [(-1) ** c * (1 << 17) for c in range(16)], [1 << 17] * 8 + [-(1 << 17)] * 7 + [0]]


def test_twin_row_at_the_bound_on_worst_case_streams(engine_lib, oracle_mod, worst16):
    """sum |m| = 2^21 against |x| = sum |q|: |v| is as large as the definition admits, and every depth clips like the reference"""
    X, S, _ = worst16
    assert sum(abs(m) for m in SATURATING[0]) == 1 << 21
    lo, hi = 0, 2048                                                        # (the Python reference walks these frames sample by sample)
    big = int(np.argmax(np.abs(X[0])))
    lo = max(0, min(big - 1024, X.shape[1] - 2048)); hi = lo + 2048
    Xs = np.ascontiguousarray(X[:, lo:hi])
    for bits, dither in ((24, "T"), (16, "R"), (32, "F"), (20, "X")):
        got = _twin_equals_ref(engine_lib, oracle_mod, Xs, S, SATURATING, bit_depth=bits, dither=dither, seed=9, first_index=lo)
        if bits == 24:
            from helpers import decode_pcm
            v = decode_pcm(got, 24, 3)
            assert v[:, 0].max() == (1 << 23) - 1 and v[:, 0].min() == -(1 << 23)      # clipped at both ends
            assert np.all(np.abs(v[:, 1]) <= 1)                                        # the alternating row cancels to the dither


def test_twin_refuses_what_create_refuses(engine_lib):
    d = engine_lib
    x = np.zeros((2, 8), dtype=np.int32)
    for kw, coef, frag in ((dict(), [[1 << 18, 0]], "above 4.0"), (dict(dither="N"), [[U, 0]], "dither"), (dict(bit_depth=12), [[U, 0]], "bit depth"),
                           (dict(capacity=8 * 3 - 1), [[U, 0]], "too small")):
        with pytest.raises(d.D2DError) as ei:
            d.mix_frames_host(x, 25, coef, **kw)
        assert frag in ei.value.message


# ---- the sanitised run ----

def test_twin_and_mix_parser_sanitised(tmp_path):
    exe = str(tmp_path / "mix_fuzz")
    src = [os.path.join(ROOT, "tools", "mix_fuzz.cpp"), os.path.join(CSRC, "mix", "d2d_mix_host.cpp")]
    cmd = ["g++", "-g", "-O1", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe] + src
    r = subprocess.run(cmd, cwd=os.path.join(ROOT, "tools"), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    p = subprocess.run([exe, "1", "300"], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "fuzz ok" in p.stdout and not p.stderr, (p.stdout[-500:], p.stderr[-3000:])
