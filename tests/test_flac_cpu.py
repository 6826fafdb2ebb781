"""The FLAC entry points that need no GPU (include/dsd2dxd_amd.h, "FLAC frames on the GPU"): d2d_flac_encode_host -- the sink's own
frame encoder behind the C ABI, the reference of tests/test_gpu_flac.py -- against the plain-Python restatement of the format in
flac_ref.py, the bound, the frame-number boundaries, and the parameter checks of d2d_flac_encode_device, which answer before any
device call."""
import ctypes as C

import numpy as np
import pytest

import flac_ref as R

CHANNELS = (1, 2, 3, 8)
DEPTHS = (16, 20, 24)
# (frames, final): three blocks with a short last one; exactly one block; verbatim last blocks of 1 and 2 samples; a last block of 3
# (a single residual); under one block and not final (0 blocks); nothing at all
LENGTHS = ((2 * 4096 + 1000, True), (4096, True), (4096 + 1, True), (4096 + 2, True), (4096 + 3, True), (4095, False), (0, True), (0, False))


def _expect_result(sizes):
    return (sum(sizes), min(sizes) if sizes else 0, max(sizes) if sizes else 0)


@pytest.mark.parametrize("signal", R.SIGNALS)
@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("channels", CHANNELS)
def test_host_encoder_equals_the_format_restatement(engine_lib, channels, depth, signal):
    for frames, final in LENGTHS:
        s = R.signal(signal, frames, channels, depth, seed=frames + channels)
        pcm = R.pack_pcm(s, depth)
        want, sizes, used = R.encode(s, depth, first_block=5, final=final)
        got, res, consumed = engine_lib.flac_encode_host(channels, depth, pcm, first_block=5, final=final)
        assert got == want, (frames, final)
        assert (res.bytes_out, res.min_frame_bytes, res.max_frame_bytes) == _expect_result(sizes), (frames, final)
        assert consumed == used
        # every frame within the documented bound
        assert len(got) <= engine_lib.flac_bound_bytes(channels, depth, frames, final)
        for i, fs in enumerate(sizes):
            assert fs <= R.frame_bound(channels, depth, min(4096, frames - 4096 * i))


# The decoder is a per-sample Python loop, so the round trip takes every signal and depth at the longest length in stereo, and every
# other channel count at the lengths with verbatim and single-residual last blocks.
ROUND_TRIP = [(2, d, s, 2 * 4096 + 1000) for d in DEPTHS for s in R.SIGNALS] + \
             [(c, d, "random", 4096 + x) for c in (1, 3, 8) for d in (16, 24) for x in (1, 2, 3)]


@pytest.mark.parametrize("channels,depth,signal,frames", ROUND_TRIP)
def test_decode_round_trip(engine_lib, channels, depth, signal, frames):
    s = R.signal(signal, frames, channels, depth, seed=7)
    got, res, _ = engine_lib.flac_encode_host(channels, depth, R.pack_pcm(s, depth), first_block=0, final=True)
    back, sizes = R.decode(got, channels, depth)              # (asserts every CRC-8 and CRC-16)
    assert np.array_equal(back, s)
    assert (res.bytes_out, res.min_frame_bytes, res.max_frame_bytes) == _expect_result(sizes)


BOUNDARIES = (0x7F, 0x7FF, 0xFFFF, 0x1FFFFF, 0x3FFFFFF)


@pytest.mark.parametrize("last_short", BOUNDARIES)
def test_frame_numbers_across_utf8_lengths(engine_lib, last_short):
    """two blocks whose numbers straddle each length boundary of the "UTF-8" coding"""
    s = R.signal("random", 2 * 4096, 1, 16, seed=last_short)
    want, _, _ = R.encode(s, 16, first_block=last_short)
    got, _, _ = engine_lib.flac_encode_host(1, 16, R.pack_pcm(s, 16), first_block=last_short)
    assert got == want
    assert len(R.utf8_number(last_short)) + 1 == len(R.utf8_number(last_short + 1))
    back, _ = R.decode(got, 1, 16, first_block=last_short)
    assert np.array_equal(back, s)


def test_last_legal_frame_number_and_refusal_beyond(engine_lib):
    s = R.signal("random", 2 * 4096, 2, 24, seed=3)
    pcm = R.pack_pcm(s, 24)
    top = (1 << 31) - 1
    got, _, _ = engine_lib.flac_encode_host(2, 24, pcm, first_block=top - 1)          # numbers 2^31 - 2 and 2^31 - 1
    assert got == R.encode(s, 24, first_block=top - 1)[0]
    assert np.array_equal(R.decode(got, 2, 24, first_block=top - 1)[0], s)
    for first in (top, 1 << 31, 0xFFFFFFFF):                                          # the second block would pass 2^31 - 1
        with pytest.raises(engine_lib.D2DError) as ei:
            engine_lib.flac_encode_host(2, 24, pcm, first_block=first)
        assert ei.value.code == -1 and "31 bits" in ei.value.message
    one = pcm[:4096 * 6]
    assert engine_lib.flac_encode_host(2, 24, one, first_block=top)[0] == R.encode(s[:4096], 24, first_block=top)[0]


def test_bound_is_the_documented_closed_form(engine_lib):
    for ch in range(1, 9):
        for depth in DEPTHS:
            for frames in (0, 1, 2, 3, 1000, 4095, 4096, 4097, 3 * 4096 + 17, 1292 * 4096 + 5):
                for final in (0, 1):
                    assert engine_lib.flac_bound_bytes(ch, depth, frames, final) == R.bound_bytes(ch, depth, frames, final)
                    blocks = frames // 4096 + (1 if final and frames % 4096 else 0)
                    slot = (R.frame_bound(ch, depth, 4096) + 15) // 16 * 16
                    assert engine_lib.flac_workspace_bytes(ch, depth, frames, final) == (4 * blocks + 15) // 16 * 16 + blocks * slot
    assert engine_lib.flac_bound_bytes(0, 24, 4096, 1) == 0 and engine_lib.flac_bound_bytes(9, 24, 4096, 1) == 0
    assert engine_lib.flac_bound_bytes(2, 32, 4096, 1) == 0


def test_capacity_one_byte_short_is_refused_and_nothing_written(engine_lib):
    L = engine_lib.lib()
    s = R.signal("silence", 4096 + 10, 2, 24)              # (the frames themselves are far smaller than the bound: the bound is what is checked)
    pcm = R.pack_pcm(s, 24)
    cap = engine_lib.flac_bound_bytes(2, 24, 4096 + 10, 1)
    out = np.full(cap, 0xA5, dtype=np.uint8)
    res = engine_lib.FlacResult(111, 222, 333)
    used = C.c_size_t(444)
    rc = L.d2d_flac_encode_host(2, 24, pcm.ctypes.data, 4096 + 10, 0, 1, out.ctypes.data, cap - 1, C.byref(res), C.byref(used))
    assert rc == -20 and b"d2d_flac_bound_bytes" in L.d2d_flac_error()
    assert (out == 0xA5).all() and (res.bytes_out, res.min_frame_bytes, res.max_frame_bytes, used.value) == (111, 222, 333, 444)
    assert L.d2d_flac_encode_host(2, 24, pcm.ctypes.data, 4096 + 10, 0, 1, out.ctypes.data, cap, C.byref(res), C.byref(used)) == 0
    assert used.value == 4096 + 10 and res.bytes_out < cap


def test_device_entry_validates_before_any_device_call(engine_lib):
    """every refusal below is decided on the host: the pointers are never dereferenced and no GPU is needed (or touched)"""
    L = engine_lib.lib()
    frames = 2 * 4096 + 5
    cap, ws = engine_lib.flac_bound_bytes(2, 24, frames, 1), engine_lib.flac_workspace_bytes(2, 24, frames, 1)

    def io(**k):
        x = engine_lib.FlacIO()
        x.pcm, x.frames, x.first_block, x.final = k.get("pcm", 0x10000), k.get("frames", frames), k.get("first_block", 0), k.get("final", 1)
        x.out, x.out_capacity_bytes, x.result = k.get("out", 0x20000), k.get("cap", cap), k.get("result", 0x30000)
        x.blocks, x.frames_consumed = 777, 888
        return (engine_lib.FlacIO * 1)(x)

    cases = [
        (dict(depth=32), {}, -1, "bit depth"),
        (dict(depth=12), {}, -1, "bit depth"),
        (dict(channels=0), {}, -1, "channel count"),
        (dict(channels=9), {}, -1, "channel count"),
        ({}, dict(pcm=0x10008), -1, "16-byte aligned"),
        ({}, dict(out=0x20004), -1, "16-byte aligned"),
        (dict(workspace=0x40008), {}, -1, "workspace"),
        ({}, dict(result=0), -1, "result"),
        ({}, dict(first_block=(1 << 31) - 2), -1, "31 bits"),
        ({}, dict(cap=cap - 1), -20, "d2d_flac_bound_bytes"),
        (dict(workspace_bytes=ws - 1), {}, -20, "workspace"),
    ]
    for call, fields, code, frag in cases:
        ios = io(**fields)
        rc = L.d2d_flac_encode_device(call.get("channels", 2), call.get("depth", 24), ios, 1, C.c_void_p(call.get("workspace", 0x40000)),
                                      call.get("workspace_bytes", ws), None)
        assert rc == code and frag in L.d2d_flac_error().decode(), (call, fields, rc, L.d2d_flac_error())
        assert (ios[0].blocks, ios[0].frames_consumed) == (777, 888)
    with pytest.raises(engine_lib.D2DError) as ei:
        engine_lib.flac_encode_device(2, 32, io(), 0x40000, ws)
    assert ei.value.code == -1
