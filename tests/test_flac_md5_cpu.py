"""STREAMINFO's MD5, the host side (include/dsd2dxd_amd.h, "STREAMINFO's MD5 on the GPU"): d2d_flac_md5_init_host / _update_host /
_final_host -- the CPU twins of the device calls, built on dsd2dxd_amd/csrc/flac/flac_md5.h, the source the kernel compiles too --
against hashlib.md5 over bytes the test builds itself (for 20 bits it does the arithmetic shift in numpy); the public state record; the
refusals; a sanitised run against the sink's own MD5 (tools/flac_md5_fuzz.cpp); the CLI's --flac-md5 without --gpu-flac.  No GPU.
tests/test_gpu_flac_md5.py holds the device calls to these twins and to hashlib."""
import ctypes as C
import hashlib
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "dsd2dxd_amd", "dsd2dxd_amd_cli")
DEPTHS = (16, 20, 24)
CHANNELS = (1, 2, 3, 8)
ERR_PARAM = -1


def hashed_bytes(pcm, depth):
    """what FLAC hashes of packed PCM (a uint8 array of whole samples): 16 / 24 bits the bytes as they are; 20 bits every 3-byte sample
    shifted right by 4 arithmetically and written again as 3 little-endian bytes"""
    pcm = np.ascontiguousarray(pcm, dtype=np.uint8)
    if depth != 20:
        return pcm.tobytes()
    b = pcm.reshape(-1, 3).astype(np.int32)
    v = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
    v = np.where(v & 0x800000, v - (1 << 24), v) >> 4                  # sign-extend the container, then the arithmetic shift
    out = np.empty((v.size, 3), dtype=np.uint8)
    out[:, 0], out[:, 1], out[:, 2] = v & 0xFF, (v >> 8) & 0xFF, (v >> 16) & 0xFF
    return out.tobytes()


def frame_bytes(channels, depth):
    return channels * (2 if depth == 16 else 3)


def record(state):
    return bytes(C.string_at(C.byref(state), C.sizeof(state)))


def test_the_20_bit_rule_of_this_file_is_an_arithmetic_shift():
    pcm = np.array([0x10, 0x32, 0x54, 0xF0, 0xFF, 0xFF, 0x00, 0x00, 0x80], dtype=np.uint8)          # 0x543210, -16, -2^23
    assert hashed_bytes(pcm, 20) == bytes([0x21, 0x43, 0x05, 0xFF, 0xFF, 0xFF, 0x00, 0x00, 0xF8])


def test_the_state_record_is_96_bytes(engine_lib):
    d = engine_lib
    assert C.sizeof(d.FlacMd5State) == 96 and C.sizeof(d.FlacMd5IO) == 16
    assert (d.FlacMd5State.bytes.offset, d.FlacMd5State.tail_bytes.offset, d.FlacMd5State.reserved.offset, d.FlacMd5State.tail.offset) == (16, 24, 28, 32)
    st = d.flac_md5_init_host(3)
    for s in st:
        assert tuple(s.h) == (0x67452301, 0xEFCDAB89, 0x98BADCFE, 0x10325476) and record(s)[16:] == bytes(80)


@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("channels", CHANNELS)
def test_host_twin_equals_hashlib_in_one_update_and_in_random_splits(engine_lib, channels, depth):
    d = engine_lib
    fb = frame_bytes(channels, depth)
    rng = np.random.default_rng(1000 * channels + depth)
    frames = 3000 // fb + 517
    pcm = rng.integers(0, 256, frames * fb, dtype=np.uint8)              # random bytes: half of the 20-bit samples are negative
    if depth == 20:
        assert (pcm.reshape(-1, 3)[:, 2] & 0x80).mean() > 0.4
    want = hashlib.md5(hashed_bytes(pcm, depth)).digest()
    one = d.flac_md5_init_host(1)[0]
    d.flac_md5_update_host(channels, depth, pcm, one)
    assert d.flac_md5_final_host(one) == want
    assert one.bytes == pcm.size and one.tail_bytes == pcm.size % 64 and one.reserved == 0
    for trial in range(6):
        cuts = np.sort(rng.integers(0, frames + 1, rng.integers(1, 40)))
        st = d.flac_md5_init_host(1)[0]
        for a, b in zip(np.r_[0, cuts], np.r_[cuts, frames]):
            d.flac_md5_update_host(channels, depth, pcm[a * fb:b * fb], st)
            assert d.flac_md5_final_host(st) == hashlib.md5(hashed_bytes(pcm[:b * fb], depth)).digest(), (trial, a, b)
        assert record(st) == record(one), trial                         # the same bytes leave the same record, however they came


def test_every_residue_and_both_sides_of_the_padding_boundary(engine_lib):
    """3 n bytes for n = 0 .. 130 as mono 24-bit: gcd(3, 64) = 1, so every residue mod 64 comes at least twice -- 183 = 2 * 64 + 55 fits
    one padding block, 120 = 64 + 56 needs a second, 192 is whole blocks, 0 is the empty message"""
    d = engine_lib
    rng = np.random.default_rng(3)
    seen = set()
    for n in range(131):
        pcm = rng.integers(0, 256, 3 * n, dtype=np.uint8)
        st = d.flac_md5_init_host(1)[0]
        d.flac_md5_update_host(1, 24, pcm, st)
        assert d.flac_md5_final_host(st) == hashlib.md5(pcm.tobytes()).digest(), n
        assert (st.bytes, st.tail_bytes) == (3 * n, 3 * n % 64) and bytes(st.tail)[:st.tail_bytes] == pcm[3 * n - 3 * n % 64:].tobytes()
        assert bytes(st.tail)[st.tail_bytes:] == bytes(64 - st.tail_bytes)
        seen.add(3 * n % 64)
    assert seen == set(range(64)) and {183 % 64, 120 % 64, 192 % 64} == {55, 56, 0}
    st = d.flac_md5_init_host(1)[0]
    assert d.flac_md5_final_host(st).hex() == "d41d8cd98f00b204e9800998ecf8427e"


def test_the_bit_count_passes_2_to_the_32(engine_lib):
    d = engine_lib
    n = (1 << 29) + 6                                                    # bytes: 8 n = 2^32 + 48 bits
    pcm = np.resize(np.random.default_rng(29).integers(0, 256, 1 << 20, dtype=np.uint8), n)
    st = d.flac_md5_init_host(1)[0]
    half = (n // 4) * 2 + 2                                              # (as mono 16-bit frames: 2^29 + 6 is no multiple of 3)
    d.flac_md5_update_host(1, 16, pcm[:half], st)
    d.flac_md5_update_host(1, 16, pcm[half:], st)
    assert st.bytes == n and 8 * n > 1 << 32
    assert d.flac_md5_final_host(st) == hashlib.md5(pcm).digest()


def test_final_leaves_the_state_unchanged_and_may_be_asked_again(engine_lib):
    d = engine_lib
    pcm = np.random.default_rng(5).integers(0, 256, 6 * 37, dtype=np.uint8)
    st = d.flac_md5_init_host(1)[0]
    d.flac_md5_update_host(2, 24, pcm[:6 * 20], st)
    before = record(st)
    first = d.flac_md5_final_host(st)
    assert record(st) == before and d.flac_md5_final_host(st) == first == hashlib.md5(pcm[:6 * 20].tobytes()).digest()
    d.flac_md5_update_host(2, 24, pcm[6 * 20:], st)                      # "the digest so far" did not end the hash
    assert d.flac_md5_final_host(st) == hashlib.md5(pcm.tobytes()).digest()
    d.flac_md5_update_host(2, 24, pcm[:0], st)                           # frames == 0: the state as it is
    assert d.flac_md5_final_host(st) == hashlib.md5(pcm.tobytes()).digest()


def test_refusals_return_err_param_and_change_nothing(engine_lib):
    d = engine_lib
    L = d.lib()
    pcm = np.arange(48, dtype=np.uint8)
    st = d.flac_md5_init_host(1)[0]
    d.flac_md5_update_host(1, 16, pcm[:10], st)
    before = record(st)
    for channels, depth, ptr, frames, text in ((2, 17, pcm.ctypes.data, 4, "bit depth"), (2, 32, pcm.ctypes.data, 4, "bit depth"),
                                               (0, 16, pcm.ctypes.data, 4, "channel"), (9, 16, pcm.ctypes.data, 1, "channel"),
                                               (2, 16, None, 4, "null pcm")):
        rc = L.d2d_flac_md5_update_host(channels, depth, ptr, frames, C.byref(st))
        assert rc == ERR_PARAM and text in L.d2d_flac_error().decode(), (channels, depth, frames)
        assert record(st) == before
    assert L.d2d_flac_md5_update_host(2, 16, pcm.ctypes.data, 4, None) == ERR_PARAM
    digest = (C.c_uint8 * 16)(*([0xEE] * 16))
    assert L.d2d_flac_md5_final_host(None, digest) == ERR_PARAM and bytes(digest) == bytes([0xEE] * 16)
    assert L.d2d_flac_md5_final_host(C.byref(st), None) == ERR_PARAM and record(st) == before


def test_host_twin_against_the_sinks_md5_sanitised(tmp_path):
    exe = str(tmp_path / "flac_md5_fuzz")
    src = [os.path.join(ROOT, "tools", "flac_md5_fuzz.cpp"), os.path.join(ROOT, "dsd2dxd_amd", "csrc", "flac", "d2d_flac_host.cpp")]
    cmd = ["g++", "-g", "-O1", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe] + src
    r = subprocess.run(cmd, cwd=os.path.join(ROOT, "tools"), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    p = subprocess.run([exe, "1", "300"], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "fuzz ok" in p.stdout and not p.stderr, (p.stdout[-500:], p.stderr[-3000:])


def test_cli_flac_md5_needs_gpu_flac(engine_lib, tmp_path):
    if not os.path.exists(CLI):
        engine_lib.build_library()
    for extra in (["-o", "f"], ["-o", "w", "--gpu-flac"], ["--gpu-flac"]):
        r = subprocess.run([CLI, "convert"] + extra + ["--flac-md5", str(tmp_path / "x.dsf")], capture_output=True, text=True)
        assert r.returncode == 2, (extra, r.stderr)
        assert r.stderr.startswith("ERROR:") and "--flac-md5" in r.stderr and r.stderr.count("\n") == 1
