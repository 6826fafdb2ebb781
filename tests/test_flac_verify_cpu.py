"""The FLAC frame parser on the host (dsd2dxd_amd/csrc/flac/flac_parse.h behind d2d_flac_decode_host and d2d_flac_verify_host, the
CPU twin of the GPU verify call): round trips of every encoder here, agreement with the Python restatements in both directions, one
crafted frame per reason of include/dsd2dxd_amd.h's D2D_FLAC_BAD_*, the refusals, a sanitised mutation run of the parser
(tools/flac_decode_fuzz.cpp) and the CLI's `verify`.  No GPU.  tests/test_gpu_flac_verify.py runs the same crafted cases on the device."""
import hashlib
import os
import subprocess

import numpy as np
import pytest

import flac_lpc_ref as P
import flac_ref as R
import flac_search_ref as S
from test_flac_lpc_cpu import CASES as LPC_CASES, ar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "dsd2dxd_amd", "dsd2dxd_amd_cli")
BLOCK = R.BLOCK
EFFORTS = (0, 1, 12)
NONE = 0xFFFFFFFF
LENGTHS = (1, 2, 15, 16, 63, 64, 4095, 4096, 4097, 2 * 4096 + 100)
(BAD_NONE, BAD_SIZE, BAD_HEADER, BAD_CRC8, BAD_CRC16, BAD_UNSUPPORTED, BAD_SYNTAX, BAD_LENGTH, BAD_SAMPLES) = range(9)


def clean(samples, blocks):
    return (samples, blocks, 0, NONE, BAD_NONE)


def nblocks(n):
    return (n + BLOCK - 1) // BLOCK


def make_signal(kind, n, ch, depth, seed):
    """the existing generators, by turns: sines, noise at several widths, a spike in noise, amplitudes that vary by block, an AR process"""
    if kind == 0:
        return R.signal("sine", n, ch, depth)
    if kind == 1:
        return R.noise(n, ch, depth, 3 + seed % (depth - 4), seed)
    if kind == 2:
        return R.spike_at(n, ch, depth, n // 2, (1 << (depth - 1)) - 1, 5)
    if kind == 3:
        return R.varying(n, ch, depth, seed)
    return R._clip(R.signal("sine", n, ch, depth) // 2 + R.noise(n, ch, depth, depth - 6, seed), depth)


@pytest.mark.parametrize("depth", (16, 20, 24))
@pytest.mark.parametrize("channels", (1, 2, 3, 8))
@pytest.mark.parametrize("effort", EFFORTS)
def test_round_trip_of_the_host_encoder(engine_lib, effort, channels, depth):
    d = engine_lib
    for i, n in enumerate(LENGTHS):
        x = make_signal((i + channels + depth) % 5, n, channels, depth, 7 * i + channels)
        pcm = R.pack_pcm(x, depth)
        frames = d.flac_encode_host(channels, depth, pcm, effort=effort)[0]
        back, frames_out, chk = d.flac_decode_host(channels, depth, frames)
        assert frames_out == n and chk.as_tuple() == clean(n, nblocks(n)), (n, chk.as_tuple())
        # byte for byte; at 20 bits the container's low nibble, which no encoder codes, comes back as zero
        want = pcm if depth != 20 else R.pack_pcm(x << 4, 24)
        assert back == want.tobytes(), n
        for sizes in (None, frame_sizes(d, channels, depth, pcm, effort)):      # walked by decoding; by the size table
            v = d.flac_verify_host(channels, depth, pcm, frames, sizes=sizes)
            assert v.as_tuple() == clean(n, nblocks(n)), (n, sizes, v.as_tuple())


def frame_sizes(d, channels, depth, pcm, effort, first_block=0):
    """the sizes of a stream's frames: frames are independent, so each block encoded by itself is its frame"""
    step = BLOCK * channels * (2 if depth == 16 else 3)
    return [len(d.flac_encode_host(channels, depth, pcm[a:a + step], first_block=first_block + i, effort=effort)[0]) for i, a in enumerate(range(0, pcm.size, step))]


@pytest.mark.parametrize("effort", EFFORTS)
def test_the_lpc_cases_round_trip(engine_lib, effort):
    d = engine_lib
    for c in LPC_CASES:
        x, depth, ch = c["samples"], c["depth"], c["samples"].shape[1]
        pcm = R.pack_pcm(x, depth)
        frames, _, used = d.flac_encode_host(ch, depth, pcm, first_block=c["first_block"], final=c["final"], effort=effort)
        back, frames_out, chk = d.flac_decode_host(ch, depth, frames, first_block=c["first_block"])
        assert frames_out == used and chk.as_tuple() == clean(used, nblocks(used)), c["name"]
        assert np.array_equal(R.unpack_pcm(np.frombuffer(back, dtype=np.uint8), ch, depth), x[:used]), c["name"]
        v = d.flac_verify_host(ch, depth, pcm, frames, first_block=c["first_block"], final=c["final"])
        assert v.as_tuple() == clean(used, nblocks(used)), c["name"]


def test_independence_from_the_python_restatements(engine_lib):
    """frames of the three Python encoders decode to the same samples through the host decoder; the host decoder and the Python
    decoders agree on the frames of the host encoder"""
    d = engine_lib
    for ch, depth, n, seed in ((2, 24, 4096 + 37, 1), (1, 16, 700, 2), (3, 20, 64, 3)):
        x = R._clip(ar(n, ch, depth, 4, seed, amp=300.0) + R.signal("sine", n, ch, depth) // 4, depth)
        pcm = R.pack_pcm(x, depth)
        for enc in (R, S, P):
            frames = enc.encode(x, depth, first_block=5)[0]
            back, frames_out, chk = d.flac_decode_host(ch, depth, frames, first_block=5)
            assert chk.as_tuple() == clean(n, nblocks(n)), (enc.__name__, chk.as_tuple())
            assert np.array_equal(R.unpack_pcm(np.frombuffer(back, dtype=np.uint8), ch, depth), x)
            assert d.flac_verify_host(ch, depth, pcm, frames, first_block=5).as_tuple() == clean(n, nblocks(n))
        for effort, dec in ((0, R), (1, S), (12, P)):
            frames = d.flac_encode_host(ch, depth, pcm, first_block=5, effort=effort)[0]
            back = d.flac_decode_host(ch, depth, frames, first_block=5)[0]
            assert np.array_equal(dec.decode(frames, ch, depth, 5)[0], R.unpack_pcm(np.frombuffer(back, dtype=np.uint8), ch, depth))


@pytest.mark.parametrize("first", (0, 127, 128, 2047, 2048, 65535, 65536, (1 << 31) - 3))
def test_frame_numbers_across_the_utf8_lengths(engine_lib, first):
    d = engine_lib
    x = R.noise(2 * BLOCK + 10, 2, 16, 6, first % 97)
    pcm = R.pack_pcm(x, 16)
    for effort in EFFORTS:
        frames = d.flac_encode_host(2, 16, pcm, first_block=first, effort=effort)[0]
        back, n, chk = d.flac_decode_host(2, 16, frames, first_block=first)
        assert back == pcm.tobytes() and chk.as_tuple() == clean(x.shape[0], 3)
        assert d.flac_verify_host(2, 16, pcm, frames, first_block=first).as_tuple() == clean(x.shape[0], 3)
    # the same frames numbered from elsewhere are not this call's
    chk = d.flac_decode_host(2, 16, frames, first_block=first + 1 if first < (1 << 31) - 3 else first - 1)[2]
    assert chk.as_tuple() == (0, 1, 1, 0, BAD_HEADER)


# ---- one crafted case per reason ----------------------------------------------------------------------------------------------------
# A 2-channel 24-bit stream of three blocks at effort 0 (independent channels, order 2, one partition: every bit position below is
# known); the middle frame is damaged.  Shared with tests/test_gpu_flac_verify.py.

CRAFT_CH, CRAFT_DEPTH, CRAFT_FIRST = 2, 24, 200              # frame numbers 200, 201, 202: two UTF-8 bytes, a header of 7 bytes
CRAFT_HEADER = 7


def craft_stream(d):
    x = R.noise(2 * BLOCK + 100, CRAFT_CH, CRAFT_DEPTH, 9, 11)
    pcm = R.pack_pcm(x, CRAFT_DEPTH)
    frames = d.flac_encode_host(CRAFT_CH, CRAFT_DEPTH, pcm, first_block=CRAFT_FIRST, effort=0)[0]
    sizes = R.decode(frames, CRAFT_CH, CRAFT_DEPTH, CRAFT_FIRST)[1]
    assert len(sizes) == 3
    return x, pcm, frames, sizes


def _bits(frame):
    return np.unpackbits(np.frombuffer(frame, dtype=np.uint8))


def _bytes(bits):
    return np.packbits(bits).tobytes()


def _fix(frame, header=True, body=True):
    f = bytearray(frame)
    if header:
        f[CRAFT_HEADER - 1] = R.crc8(bytes(f[:CRAFT_HEADER - 1]))
    if body:
        f[-2:] = R.crc16(bytes(f[:-2])).to_bytes(2, "big")
    return bytes(f)


def _set(frame, bit, width, value):
    b = _bits(frame).copy()
    b[bit:bit + width] = [(value >> (width - 1 - i)) & 1 for i in range(width)]
    return _bytes(b)


def _second_subframe_end(frame):
    """the bit behind the last Rice code of the frame's second subframe = the first padding bit"""
    b = _bits(frame)
    pos = 8 * CRAFT_HEADER
    for _ in range(CRAFT_CH):
        pos += 8 + 2 * CRAFT_DEPTH + 6                       # subframe header, two warm-up samples, method and partition order
        k = int("".join(map(str, b[pos:pos + 5])), 2)
        pos += 5
        for _ in range(BLOCK - 2):
            pos += int(np.argmax(b[pos:])) + 1 + k
    return pos


# the first subframe of the middle frame starts at bit 56: 0 001010 0 | 24 + 24 warm-up | 01 0000 | kkkkk | codes
SUB0 = 8 * CRAFT_HEADER
RICE0 = SUB0 + 8 + 2 * CRAFT_DEPTH


def mutations(frame):
    """name -> (the damaged middle frame, the reason it must get)"""
    k0 = int("".join(map(str, _bits(frame)[RICE0 + 6:RICE0 + 11])), 2)
    end = _second_subframe_end(frame)
    assert end % 8 != 0 and (end + 7) // 8 == len(frame) - 2, "the crafted stream needs padding bits in its middle frame"
    m = {}
    m["payload bit"] = (_set(frame, 8 * (len(frame) // 2), 1, 1 - int(_bits(frame)[8 * (len(frame) // 2)])), BAD_CRC16)
    # the sample-rate code is the one header field whose other values are valid FLAC, not a field "that is not this call's": a flipped
    # bit there is not HEADER's, so the CRC-8 is what notices it
    m["header bit"] = (_set(frame, 20 + 3, 1, 1), BAD_CRC8)
    m["frame number"] = (_fix(_set(frame, 8 * 5 + 7, 1, 1 - int(_bits(frame)[8 * 5 + 7])), body=False), BAD_HEADER)
    m["depth code"] = (_fix(_set(frame, 28, 3, 4), body=False), BAD_HEADER)
    m["constant subframe"] = (_fix(_set(frame, SUB0 + 1, 6, 0)), BAD_UNSUPPORTED)
    m["reserved subframe type"] = (_fix(_set(frame, SUB0 + 1, 6, 0b000100)), BAD_SYNTAX)
    m["partition order"] = (_fix(_set(frame, RICE0 + 2, 4, 13)), BAD_SYNTAX)          # 4096 % 2^13 != 0
    # the last bit of the frame's last Rice code (k > 0: a low bit of the residual)
    m["residual bit"] = (_fix(_set(frame, end - 1, 1, 1 - int(_bits(frame)[end - 1]))), BAD_SAMPLES)
    # a Rice parameter that is not the codes': they overrun the frame (the bits run out) or underrun it (the subframes end early)
    m["rice parameter up"] = (_fix(_set(frame, RICE0 + 6, 5, k0 + 3)), (BAD_SYNTAX, BAD_LENGTH))
    m["rice parameter down"] = (_fix(_set(frame, RICE0 + 6, 5, k0 - 2)), (BAD_SYNTAX, BAD_LENGTH))
    m["padding"] = (_fix(_set(frame, end, 1, 1)), BAD_LENGTH)
    return m, k0


@pytest.fixture(scope="module")
def crafted(engine_lib):
    x, pcm, frames, sizes = craft_stream(engine_lib)
    a, b = sizes[0], sizes[0] + sizes[1]
    muts, k0 = mutations(frames[a:b])
    assert k0 >= 2
    return dict(x=x, pcm=pcm, frames=frames, sizes=sizes, muts=muts, k0=k0)


def damaged(c, name):
    a, b = c["sizes"][0], c["sizes"][0] + c["sizes"][1]
    frame = c["muts"][name][0]
    assert len(frame) == b - a and frame != c["frames"][a:b]
    return c["frames"][:a] + frame + c["frames"][b:]


MUTATIONS = ("payload bit", "header bit", "frame number", "depth code", "constant subframe", "reserved subframe type", "partition order",
             "residual bit", "rice parameter up", "rice parameter down", "padding")


@pytest.mark.parametrize("name", MUTATIONS)
def test_one_crafted_frame_per_reason(engine_lib, crafted, name):
    d, c = engine_lib, crafted
    out = damaged(c, name)
    reason = c["muts"][name][1]
    good = c["x"].shape[0] - BLOCK
    v = d.flac_verify_host(CRAFT_CH, CRAFT_DEPTH, c["pcm"], out, first_block=CRAFT_FIRST, sizes=c["sizes"])
    assert v.as_tuple()[:4] == (good, 3, 1, 1), (name, v.as_tuple())         # blocks 0 and 2 are still good
    assert v.first_bad_reason in (reason if isinstance(reason, tuple) else (reason,)), (name, v.as_tuple())
    # the decoder, which has no size table and no PCM, stops at the same block
    back, n, chk = d.flac_decode_host(CRAFT_CH, CRAFT_DEPTH, out, first_block=CRAFT_FIRST)
    if reason != BAD_SAMPLES:                                                # (a wrong residual still decodes: to other samples)
        assert n == BLOCK and chk.bad_blocks == 1 and chk.first_bad_block == 1 and back == c["pcm"].tobytes()[:BLOCK * 6], name
        if reason in (BAD_HEADER, BAD_CRC8, BAD_UNSUPPORTED):
            assert chk.first_bad_reason == reason
    else:
        assert n == c["x"].shape[0] and chk.bad_blocks == 0 and back != c["pcm"].tobytes()


def test_a_wrong_size_entry(engine_lib, crafted):
    """rule 1: an entry of 0, or one above the frame bound, is SIZE at its block; the frames behind it are no longer where the table
    says, so the last block is bad too (HEADER: another frame's bytes; or SIZE: it does not end at bytes_out).  Walking the same
    bytes without the table finds all three frames good."""
    d, c = engine_lib, crafted
    good = c["x"].shape[0]
    for wrong in (0, R.frame_bound(CRAFT_CH, CRAFT_DEPTH, BLOCK) + 1):
        sizes = list(c["sizes"])
        sizes[1] = wrong
        v = d.flac_verify_host(CRAFT_CH, CRAFT_DEPTH, c["pcm"], c["frames"], first_block=CRAFT_FIRST, sizes=sizes)
        assert v.as_tuple() == (BLOCK, 3, 2, 1, BAD_SIZE), v.as_tuple()
    sizes = list(c["sizes"])
    sizes[1] -= 1                                            # a plausible size that is not the frame's: its CRC-16 is elsewhere
    v = d.flac_verify_host(CRAFT_CH, CRAFT_DEPTH, c["pcm"], c["frames"], first_block=CRAFT_FIRST, sizes=sizes)
    assert v.as_tuple() == (BLOCK, 3, 2, 1, BAD_CRC16), v.as_tuple()
    assert d.flac_verify_host(CRAFT_CH, CRAFT_DEPTH, c["pcm"], c["frames"], first_block=CRAFT_FIRST).as_tuple() == clean(good, 3)


def test_a_changed_pcm_sample_with_untouched_frames(engine_lib, crafted):
    d, c = engine_lib, crafted
    for frame_index, channel in ((BLOCK + 17, 1), (2 * BLOCK + 99, 0), (0, 0)):
        pcm = c["pcm"].copy()
        pcm[(frame_index * CRAFT_CH + channel) * 3] ^= 1
        block = frame_index // BLOCK
        n = (BLOCK, BLOCK, 100)[block]
        for sizes in (c["sizes"], None):
            v = d.flac_verify_host(CRAFT_CH, CRAFT_DEPTH, pcm, c["frames"], first_block=CRAFT_FIRST, sizes=sizes)
            assert v.as_tuple() == (c["x"].shape[0] - n, 3, 1, block, BAD_SAMPLES), (frame_index, v.as_tuple())


# ---- refusals ---------------------------------------------------------------------------------------------------------------------

def test_refusals_have_the_codes_and_messages_of_the_encode_calls(engine_lib, crafted):
    d, c = engine_lib, crafted
    for call in (lambda ch, depth: d.flac_decode_host(ch, depth, c["frames"]), lambda ch, depth: d.flac_verify_host(ch, depth, c["pcm"], c["frames"])):
        for ch, depth, text in ((2, 12, "Invalid bit depth"), (2, 32, "Invalid bit depth"), (0, 24, "Invalid channel count"), (9, 24, "Invalid channel count")):
            with pytest.raises(d.D2DError) as ei:
                call(ch, depth)
            assert ei.value.code == -1 and text in ei.value.message
    with pytest.raises(d.D2DError) as ei:
        d.flac_verify_host(CRAFT_CH, CRAFT_DEPTH, c["pcm"], c["frames"], first_block=(1 << 31) - 2)
    assert ei.value.code == -1 and "31 bits" in ei.value.message
    # a pcm buffer a byte short: D2D_ERR_CAPACITY, and not a byte of it is written
    need = c["x"].shape[0] * 6
    guard = np.full(need + 64, 0x5A, dtype=np.uint8)
    with pytest.raises(d.D2DError) as ei:
        d.flac_decode_host(CRAFT_CH, CRAFT_DEPTH, c["frames"], first_block=CRAFT_FIRST, capacity=need - 1, pcm=guard)
    assert ei.value.code == -20 and (guard == 0x5A).all()
    back, n, chk = d.flac_decode_host(CRAFT_CH, CRAFT_DEPTH, c["frames"], first_block=CRAFT_FIRST, capacity=need, pcm=guard)
    assert n == c["x"].shape[0] and (guard[need:] == 0x5A).all() and back == c["pcm"].tobytes()      # exactly [0, frames_out * frame_bytes)


# ---- the parser on damaged bytes, sanitised -------------------------------------------------------------------------------------------

def test_the_parser_reads_within_bounds_on_mutated_frames(tmp_path):
    exe = str(tmp_path / "flac_decode_fuzz")
    src = [os.path.join(ROOT, "tools", "flac_decode_fuzz.cpp"), os.path.join(ROOT, "dsd2dxd_amd", "csrc", "flac", "d2d_flac_host.cpp")]
    cmd = ["g++", "-g", "-O1", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe] + src
    r = subprocess.run(cmd, cwd=os.path.join(ROOT, "tools"), capture_output=True, text=True)
    if r.returncode != 0 and "sanitize" in r.stderr:
        pytest.skip("sanitizer runtime not available: " + r.stderr[-200:])
    assert r.returncode == 0, r.stderr[-2000:]
    p = subprocess.run([exe, "1", "2000"], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "fuzz ok" in p.stdout and not p.stderr, (p.stdout[-500:], p.stderr[-3000:])
    reached = {line.split()[1]: int(line.split()[2]) for line in p.stdout.splitlines() if line.startswith("reached ")}
    assert sum(reached.values()) == 2000
    for reason in ("SYNTAX", "LENGTH", "SAMPLES", "UNSUPPORTED", "CRC8", "CRC16", "HEADER", "SIZE"):
        assert reached[reason] >= 1, reached


# ---- the CLI's verify --------------------------------------------------------------------------------------------------------------

def flac_file(d, x, depth, effort, rate=88200):
    """the file the host sink writes for these samples: fLaC, STREAMINFO with the MD5 of the samples, the frames"""
    ch = x.shape[1]
    pcm = R.pack_pcm(x, depth)
    frames = d.flac_encode_host(ch, depth, pcm, effort=effort)[0]
    sizes = P.decode(frames, ch, depth)[1]
    hashed = pcm.tobytes() if depth != 20 else (x & 0xFFFFFF).astype("<u4").view(np.uint8).reshape(-1, 4)[:, :3].tobytes()
    si = bytearray(34)
    si[0:2] = si[2:4] = BLOCK.to_bytes(2, "big")
    si[4:7], si[7:10] = min(sizes).to_bytes(3, "big"), max(sizes).to_bytes(3, "big")
    si[10:18] = ((rate << 44) | ((ch - 1) << 41) | ((depth - 1) << 36) | x.shape[0]).to_bytes(8, "big")
    si[18:34] = hashlib.md5(hashed).digest()
    return b"fLaC" + bytes([0x80, 0, 0, 34]) + bytes(si) + frames


def test_cli_verify(engine_lib, tmp_path):
    if not os.path.exists(CLI):
        engine_lib.build_library()
    d = engine_lib
    names = {}
    for effort, depth, ch in ((0, 24, 2), (1, 16, 1), (12, 20, 3)):
        x = R._clip(ar(BLOCK + 300, ch, depth, 4, effort + 1) + R.signal("sine", BLOCK + 300, ch, depth) // 4, depth)
        blob = flac_file(d, x, depth, effort)
        for kind in ("good", "nomd5", "flipped", "md5"):
            b = bytearray(blob)
            if kind == "nomd5":
                b[26:42] = bytes(16)
            elif kind == "flipped":
                b[42 + 3000] ^= 0x10                         # one audio byte of the first frame
            elif kind == "md5":
                b[30] ^= 1
            names[(effort, kind)] = str(tmp_path / f"e{effort}_{kind}.flac")
            open(names[(effort, kind)], "wb").write(b)
    for effort in EFFORTS:
        r = subprocess.run([CLI, "verify", names[(effort, "good")], names[(effort, "nomd5")]], capture_output=True, text=True)
        lines = r.stdout.splitlines()
        assert r.returncode == 0 and lines[0].endswith(": ok") and lines[1].endswith(": ok (no MD5 in STREAMINFO)"), (r.stdout, r.stderr)
        r = subprocess.run([CLI, "verify", names[(effort, "flipped")]], capture_output=True, text=True)
        assert r.returncode != 0 and "block 0" in r.stdout and "CRC16" in r.stdout, r.stdout
        r = subprocess.run([CLI, "verify", names[(effort, "md5")]], capture_output=True, text=True)
        assert r.returncode != 0 and "MD5" in r.stdout, r.stdout
        # a good file does not hide a bad one
        r = subprocess.run([CLI, "verify", names[(effort, "good")], names[(effort, "flipped")]], capture_output=True, text=True)
        assert r.returncode != 0 and r.stdout.splitlines()[0].endswith(": ok")
