"""The cooperative FLAC verifier on the host (dsd2dxd_amd/csrc/flac/flac_expect.h behind d2d_flac_verify_host_method, the CPU twin of
flac_verify_coop_kernel): whatever the method, the record is the serial parser's; what differs is who decided a block, and
d2d_flac_verify_stats counts it.  Clean streams of every encoder must be accepted by the fast path block for block (a fast path that
always falls back fails here); every damaged frame -- the crafted ones of tests/test_flac_verify_cpu.py, every single-bit flip of three
small frames, with and without repaired CRCs -- must reach the serial parser and get its reason; frames the parser accepts and no
encoder here writes must get the same record from both methods, whichever path decides.  A sanitised mutation run
(tools/flac_coop_fuzz.cpp) holds the rule's reads inside the frame.  No GPU.  tests/test_gpu_flac_coop.py runs the same cases on the
device and imports them from here."""
import os
import subprocess

import numpy as np
import pytest

import flac_lpc_ref as P
import flac_ref as R
import flac_search_ref as S
from test_flac_lpc_cpu import CASES as LPC_CASES
from test_flac_verify_cpu import (BAD_NONE, BAD_SAMPLES, BLOCK, CRAFT_CH, CRAFT_DEPTH, CRAFT_FIRST, EFFORTS, LENGTHS, MUTATIONS, clean, craft_stream, damaged,
                                  frame_sizes, make_signal, mutations, nblocks)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AUTO, SERIAL, COOP = 0, 1, 2


def both(d, channels, depth, pcm, out, first_block=0, final=True, sizes=None):
    """(SERIAL's record, COOP's record, COOP's (fast_blocks, fallback_blocks)); AUTO must be COOP, and SERIAL's stats say so"""
    st_s, st_c, st_a = d.FlacVerifyStats(), d.FlacVerifyStats(), d.FlacVerifyStats()
    kw = dict(first_block=first_block, final=final, sizes=sizes)
    s = d.flac_verify_host(channels, depth, pcm, out, method=SERIAL, stats=st_s, **kw).as_tuple()
    c = d.flac_verify_host(channels, depth, pcm, out, method=COOP, stats=st_c, **kw).as_tuple()
    a = d.flac_verify_host(channels, depth, pcm, out, method=AUTO, stats=st_a, **kw).as_tuple()
    assert (a, st_a.as_tuple()) == (c, st_c.as_tuple())
    assert st_s.as_tuple() == (0, s[1]) and sum(st_c.as_tuple()) == c[1]
    return s, c, st_c.as_tuple()


# ---- clean streams: the fast path accepts every block of every encoder ----------------------------------------------------------------------

@pytest.mark.parametrize("depth", (16, 20, 24))
@pytest.mark.parametrize("channels", (1, 2, 3, 8))
@pytest.mark.parametrize("effort", EFFORTS)
def test_clean_streams_are_accepted_by_the_fast_path(engine_lib, effort, channels, depth):
    d = engine_lib
    for i, n in enumerate(LENGTHS):
        x = make_signal((i + channels + depth) % 5, n, channels, depth, 7 * i + channels)
        pcm = R.pack_pcm(x, depth)
        frames = d.flac_encode_host(channels, depth, pcm, first_block=126 + i, effort=effort)[0]
        sizes = frame_sizes(d, channels, depth, pcm, effort, first_block=126 + i)
        s, c, st = both(d, channels, depth, pcm, frames, first_block=126 + i, sizes=sizes)
        assert s == c == clean(n, nblocks(n)), (n, s, c)
        assert st == (nblocks(n), 0), (n, st)


@pytest.mark.parametrize("effort", EFFORTS)
def test_the_lpc_cases_are_accepted_by_the_fast_path(engine_lib, effort):
    d = engine_lib
    for case in LPC_CASES:
        x, depth, ch = case["samples"], case["depth"], case["samples"].shape[1]
        pcm = R.pack_pcm(x, depth)
        frames, _, used = d.flac_encode_host(ch, depth, pcm, first_block=case["first_block"], final=case["final"], effort=effort)
        sizes = P.decode(frames, ch, depth, case["first_block"])[1]
        s, c, st = both(d, ch, depth, pcm, frames, first_block=case["first_block"], final=case["final"], sizes=sizes)
        assert s == c == clean(used, nblocks(used)), case["name"]
        assert st == (nblocks(used), 0), (case["name"], st)


def test_the_python_encoders_frames_are_accepted_by_the_fast_path(engine_lib):
    d = engine_lib
    for ch, depth, n, seed in ((2, 24, 4096 + 37, 1), (1, 16, 700, 2), (3, 20, 64, 3)):
        x = make_signal(4, n, ch, depth, seed)
        pcm = R.pack_pcm(x, depth)
        for enc in (R, S, P):
            frames, sizes = enc.encode(x, depth, first_block=5)[:2]
            s, c, st = both(d, ch, depth, pcm, frames, first_block=5, sizes=sizes)
            assert s == c == clean(n, nblocks(n)) and st == (nblocks(n), 0), (enc.__name__, s, c, st)


def test_without_a_size_table_every_block_is_the_serial_parsers(engine_lib):
    d = engine_lib
    x = make_signal(0, BLOCK + 50, 2, 16, 1)
    pcm = R.pack_pcm(x, 16)
    frames = d.flac_encode_host(2, 16, pcm, effort=12)[0]
    s, c, st = both(d, 2, 16, pcm, frames)
    assert s == c == clean(BLOCK + 50, 2) and st == (0, 2)


# ---- the largest frame: the LDS worst case of the kernel (tests/test_gpu_flac_coop.py verifies it on the device) --------------------------------

def largest_frame_signal():
    """eight channels at 24 bits, alternating full scale: order-2 residuals of 2^25, codes of 27 and 28 bits against the bound's 30"""
    return R.signal("alternate", BLOCK, 8, 24), 0


def test_the_largest_frame_nearly_fills_the_bound(engine_lib):
    d = engine_lib
    x, effort = largest_frame_signal()
    pcm = R.pack_pcm(x, 24)
    frame = d.flac_encode_host(8, 24, pcm, effort=effort)[0]
    bound = R.frame_bound(8, 24, BLOCK)
    print("largest frame: %d of %d bytes = %.4f" % (len(frame), bound, len(frame) / bound))
    assert 0.9 * bound <= len(frame) <= bound
    s, c, st = both(d, 8, 24, pcm, frame, sizes=[len(frame)])
    assert s == c == clean(BLOCK, 1) and st == (1, 0)


# ---- damaged frames reach the serial parser -----------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def crafted(engine_lib):
    x, pcm, frames, sizes = craft_stream(engine_lib)
    a, b = sizes[0], sizes[0] + sizes[1]
    return dict(x=x, pcm=pcm, frames=frames, sizes=sizes, muts=mutations(frames[a:b])[0])


@pytest.mark.parametrize("name", MUTATIONS)
def test_crafted_mutations(engine_lib, crafted, name):
    d, c = engine_lib, crafted
    out = damaged(c, name)
    reason = c["muts"][name][1]
    s, co, st = both(d, CRAFT_CH, CRAFT_DEPTH, c["pcm"], out, first_block=CRAFT_FIRST, sizes=c["sizes"])
    assert s == co and s[:4] == (c["x"].shape[0] - BLOCK, 3, 1, 1) and s[4] in (reason if isinstance(reason, tuple) else (reason,)), (name, s, co)
    assert st == (2, 1), (name, st)


def wrong_size_tables(c):
    """[(sizes, the blocks the table puts out of place)]"""
    out = []
    for wrong in (0, R.frame_bound(CRAFT_CH, CRAFT_DEPTH, BLOCK) + 1, c["sizes"][1] - 1):
        sizes = list(c["sizes"])
        sizes[1] = wrong
        out.append((sizes, 2))
    return out


def test_wrong_size_entries_and_changed_pcm(engine_lib, crafted):
    d, c = engine_lib, crafted
    for sizes, bad in wrong_size_tables(c):
        s, co, st = both(d, CRAFT_CH, CRAFT_DEPTH, c["pcm"], c["frames"], first_block=CRAFT_FIRST, sizes=sizes)
        assert s == co and s[:4] == (BLOCK, 3, bad, 1), (sizes, s, co)
        assert st == (1, 2), (sizes, st)
    for frame_index, channel in ((BLOCK + 17, 1), (2 * BLOCK + 99, 0), (0, 0)):
        pcm = c["pcm"].copy()
        pcm[(frame_index * CRAFT_CH + channel) * 3] ^= 1
        block = frame_index // BLOCK
        s, co, st = both(d, CRAFT_CH, CRAFT_DEPTH, pcm, c["frames"], first_block=CRAFT_FIRST, sizes=c["sizes"])
        assert s == co == (c["x"].shape[0] - (BLOCK, BLOCK, 100)[block], 3, 1, block, BAD_SAMPLES), (frame_index, s, co)
        assert st == (2, 1), (frame_index, st)


# ---- every single-bit flip of three small frames -----------------------------------------------------------------------------------------------
# Stereo, 16 bits, n = 80: the search runs (n >= 16), LPC runs (n >= 64), partition orders 0 .. 2 are open (80 = 16 * 5).  One frame per
# effort, the only block of a final stream; the effort-12 frame codes a side channel.

FLIP_N, FLIP_FIRST = 80, 3
FLIP_HEADER = 4 + 1 + 2 + 1                                  # one UTF-8 byte, the block size in 16 bits


def flip_frames(d):
    """{effort: (pcm, frame)}"""
    rng = np.random.default_rng(5)
    i = np.arange(FLIP_N)
    left = np.rint(9000 * np.sin(2 * np.pi * i / 23.0)).astype(np.int64) + rng.integers(-40, 41, FLIP_N)
    x = np.stack([left, left + rng.integers(-6, 7, FLIP_N)], axis=1)          # nearly equal channels: a side channel pays
    pcm = R.pack_pcm(x, 16)
    out = {}
    for effort in EFFORTS:
        frame = d.flac_encode_host(2, 16, pcm, first_block=FLIP_FIRST, effort=effort)[0]
        assert len(frame) < 400
        out[effort] = (pcm, frame)
    assert out[12][1][3] >> 4 >= 8, "the effort-12 frame should take a stereo assignment with a side channel"
    return out


def repair(frame):
    f = bytearray(frame)
    f[FLIP_HEADER - 1] = R.crc8(bytes(f[:FLIP_HEADER - 1]))
    f[-2:] = R.crc16(bytes(f[:-2])).to_bytes(2, "big")
    return bytes(f)


def flip_corpus(frame, repaired):
    """every frame that differs from `frame` in one bit (with both CRCs put right again: one bit and the CRC fields)"""
    out = []
    for bit in range(8 * len(frame)):
        f = bytearray(frame)
        f[bit >> 3] ^= 0x80 >> (bit & 7)
        f = repair(f) if repaired else bytes(f)
        if f != frame:                                       # (a repaired flip inside a CRC field is the frame again)
            out.append((bit, f))
    return out


@pytest.mark.parametrize("repaired", (True, False))
@pytest.mark.parametrize("effort", EFFORTS)
def test_every_single_bit_flip(engine_lib, effort, repaired):
    d = engine_lib
    pcm, frame = flip_frames(d)[effort]
    s, c, st = both(d, 2, 16, pcm, frame, first_block=FLIP_FIRST, sizes=[len(frame)])
    assert s == c == clean(FLIP_N, 1) and st == (1, 0)
    corpus = flip_corpus(frame, repaired)
    assert len(corpus) >= 8 * (len(frame) - 3)
    reasons = set()
    for bit, f in corpus:
        s, c, st = both(d, 2, 16, pcm, f, first_block=FLIP_FIRST, sizes=[len(f)])
        assert s == c and st == (0, 1) and s[:4] == (0, 1, 1, 0) and s[4] != BAD_NONE, (bit, s, c, st)
        reasons.add(s[4])
    if repaired:
        assert BAD_SAMPLES in reasons and len(reasons) >= 4, reasons      # rules 6 to 8 are reached
    else:
        assert reasons <= {2, 3, 4}, reasons                 # HEADER, CRC8, CRC16


# ---- frames the parser accepts and the encoders never write ----------------------------------------------------------------------------------------

def rice_partitions(r, n, order, porder, ks=None):
    parts = S._partitions(n, order, porder)
    ks = ks or [R.rice_parameter(int(np.abs(r[lo - order:hi - order]).sum()), max(hi - lo, 1)) for lo, hi in parts]
    out = [R._bits(0b01, 2), R._bits(porder, 4)]
    for (lo, hi), k in zip(parts, ks):
        out.append(R._bits(k, 5))
        if hi > lo:
            out.append(S._rice_bits(S._zigzag(r[lo - order:hi - order]), k))
    return out


def fixed_subframe(x, bps, order, porder):
    r = x.astype(np.int64)
    for _ in range(order):
        r = r[1:] - r[:-1]
    mask = (1 << bps) - 1
    return np.concatenate([R._bits((8 | order) << 1, 8)] + [R._bits(int(v) & mask, bps) for v in x[:order]] + rice_partitions(r, len(x), order, porder))


def lpc_subframe(x, bps, q, shift, precision, porder, ks=None):
    order, mask = len(q), (1 << bps) - 1
    r = P.residuals(x.astype(np.int64), np.asarray(q, dtype=np.int64), shift)
    out = [R._bits((0x20 | (order - 1)) << 1, 8)] + [R._bits(int(v) & mask, bps) for v in x[:order]]
    out += [R._bits(precision - 1, 4), R._bits(shift, 5)] + [R._bits(int(v) & ((1 << precision) - 1), precision) for v in q]
    return np.concatenate(out + rice_partitions(r, len(x), order, porder, ks))


def frame_of(subframes, n, channels, depth, number, nibble=None):
    hdr = bytearray([0xFF, 0xF8, 0xC0 if n == BLOCK else 0x70, ((channels - 1 if nibble is None else nibble) << 4) | (R.SIZE_CODE[depth] << 1)])
    hdr += R.utf8_number(number)
    if n != BLOCK:
        hdr += (n - 1).to_bytes(2, "big")
    hdr.append(R.crc8(hdr))
    data = bytes(hdr) + np.packbits(np.concatenate(subframes)).tobytes()
    return data + R.crc16(data).to_bytes(2, "big")


def unusual_frames():
    """[(name, channels, depth, samples (n, channels), frame number, frame, the path that must decide it: 'fast', 'serial' or None)]"""
    out = []
    x = make_signal(4, BLOCK, 1, 16, 3)
    for p in (7, 8, 12):                                     # partition orders above the encoders' 6: 4096 = 2^12
        out.append(("fixed order %d, partition order %d" % (1 if p == 12 else 2, p), 1, 16, x, 9,
                    frame_of([fixed_subframe(x[:, 0], 16, 1 if p == 12 else 2, p)], BLOCK, 1, 16, 9), "serial"))
    out.append(("fixed order 4, partition order 6", 1, 16, x, 9, frame_of([fixed_subframe(x[:, 0], 16, 4, 6)], BLOCK, 1, 16, 9), "fast"))
    x = make_signal(4, 320, 2, 24, 5)
    for order, precision, shift in ((1, 2, 0), (2, 5, 3), (7, 15, 15), (32, 9, 8), (3, 13, 10)):
        rng = np.random.default_rng(order)
        top = (1 << (precision - 1)) - 1
        q = [int(v) for v in rng.integers(-top - 1, top + 1, order)]
        if order == 3:
            q = [3 << 10, -(3 << 10), 1 << 10]               # fixed order 3 as an LPC subframe
        subs = [lpc_subframe(x[:, c], 24, q, shift, precision, c) for c in range(2)]
        r = max(int(np.abs(P.residuals(x[:, c], np.asarray(q, dtype=np.int64), shift)).max()) for c in range(2))
        out.append(("LPC order %d, precision %d, shift %d" % (order, precision, shift), 2, 24, x, 130, frame_of(subs, 320, 2, 24, 130),
                    "fast" if r < 1 << 31 else "serial"))
    # left/side with LPC on the 25-bit side channel
    side = x[:, 0] - x[:, 1]
    subs = [fixed_subframe(x[:, 0], 24, 0, 0), lpc_subframe(side, 25, [1 << 9], 9, 11, 2)]
    out.append(("left/side, order-0 left, LPC side", 2, 24, x, 130, frame_of(subs, 320, 2, 24, 130, nibble=8), "fast"))
    # predictions that miss by 2^35: residuals whose zigzag leaves 32 bits, Rice parameter 30 -- valid FLAC, beyond the fast path (E3)
    x = (np.arange(16, dtype=np.int64)[:, None] % 2 * 2 - 1) * (1 << 22)
    out.append(("residuals beyond 32 bits", 1, 24, x, 0, frame_of([lpc_subframe(x[:, 0], 24, [8191], 0, 14, 0, ks=[30])], 16, 1, 24, 0), "serial"))
    return out


UNUSUAL = unusual_frames()


@pytest.mark.parametrize("case", UNUSUAL, ids=[u[0] for u in UNUSUAL])
def test_frames_the_encoders_never_write(engine_lib, case):
    d = engine_lib
    name, ch, depth, x, number, frame, path = case
    pcm = R.pack_pcm(x, depth)
    dec = P.decode(frame, ch, depth, number)                 # (the decoder of flac_lpc_ref.py is general in orders and partition orders)
    assert np.array_equal(dec[0], x), name                   # the Python decoder reads it: it is the frame it was meant to be
    s, c, st = both(d, ch, depth, pcm, frame, first_block=number, sizes=[len(frame)])
    assert s == c == clean(x.shape[0], 1), (name, s, c)
    assert path is None or st == ((1, 0) if path == "fast" else (0, 1)), (name, st)
    # ... and one changed PCM sample is SAMPLES under both
    pcm[0] ^= 1
    s, c, st = both(d, ch, depth, pcm, frame, first_block=number, sizes=[len(frame)])
    assert s == c == (0, 1, 1, 0, BAD_SAMPLES) and st == (0, 1), (name, s, c, st)


# ---- refusals ---------------------------------------------------------------------------------------------------------------------

def test_an_unknown_method_is_refused_and_nothing_written(engine_lib, crafted):
    import ctypes as C
    d, c = engine_lib, crafted
    L = d.lib()
    pcm, out = c["pcm"], np.frombuffer(c["frames"], dtype=np.uint8)
    sizes = np.array(c["sizes"], dtype=np.uint32)
    for method in (3, 7, 0xFFFFFFFF):
        chk = (C.c_uint8 * 24)(*([0x5A] * 24))
        st = (C.c_uint8 * 8)(*([0x5A] * 8))
        rc = L.d2d_flac_verify_host_method(CRAFT_CH, CRAFT_DEPTH, pcm.ctypes.data, c["x"].shape[0], CRAFT_FIRST, 1, out.ctypes.data, out.size,
                                           sizes.ctypes.data, C.cast(chk, C.POINTER(d.FlacCheck)), method, C.cast(st, C.POINTER(d.FlacVerifyStats)))
        assert rc == -1 and b"verify method" in L.d2d_flac_error()
        assert bytes(chk) == b"\x5A" * 24 and bytes(st) == b"\x5A" * 8
        with pytest.raises(d.D2DError) as ei:
            d.flac_verify_host(CRAFT_CH, CRAFT_DEPTH, pcm, c["frames"], first_block=CRAFT_FIRST, sizes=c["sizes"], method=method)
        assert ei.value.code == -1


# ---- the two methods on damaged bytes, sanitised -------------------------------------------------------------------------------------------

def test_the_two_methods_agree_on_mutated_frames_sanitised(tmp_path):
    exe = str(tmp_path / "flac_coop_fuzz")
    src = [os.path.join(ROOT, "tools", "flac_coop_fuzz.cpp"), os.path.join(ROOT, "dsd2dxd_amd", "csrc", "flac", "d2d_flac_host.cpp")]
    cmd = ["g++", "-g", "-O1", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe] + src
    r = subprocess.run(cmd, cwd=os.path.join(ROOT, "tools"), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    p = subprocess.run([exe, "1", "3000"], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "fuzz ok" in p.stdout and not p.stderr, (p.stdout[-500:], p.stderr[-3000:])
    counts = {line.split()[0]: int(line.split()[1]) for line in p.stdout.splitlines() if line.split() and line.split()[0] in ("fast", "fallback", "mutations")}
    assert counts["mutations"] == 3000 and counts["fast"] > 0 and counts["fallback"] >= 1500, counts      # (a mutation may leave the frame as it was)
