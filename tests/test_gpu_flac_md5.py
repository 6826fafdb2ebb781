"""STREAMINFO's MD5 on the GPU (include/dsd2dxd_amd.h: d2d_flac_md5_init_device / _update_device / _final_device, the stream driver
d2d_convert_stream_flac_md5 and the CLI's --flac-md5).  The reference of every digest is hashlib.md5 over bytes this test builds (the
20-bit shift in numpy: test_flac_md5_cpu.hashed_bytes); the state records are held to the host twins', which tests/test_flac_md5_cpu.py
holds to hashlib.  Every call hashes a few KB per file: the whole file is a few hundred launches."""
import ctypes as C
import hashlib
import os
import subprocess

import numpy as np
import pytest

from helpers import pack_layout, synth, write_dsf
from test_flac_md5_cpu import CHANNELS, DEPTHS, frame_bytes, hashed_bytes, record
from test_gpu_containment import Arena, describe, fill_bytes, violations

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "dsd2dxd_amd", "dsd2dxd_amd_cli")
S = 6144            # the bytes of PCM one trip of the update kernel stages: STAGE in dsd2dxd_amd/csrc/flac/d2d_flac_md5.hip
MAXF = 128          # the files of one launch: MAXF there
ERR_PARAM = -1
EMPTY = np.zeros(0, dtype=np.uint8)


def _dev(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    assert t.data_ptr() % 16 == 0
    return t


def _host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


def upload(pieces):
    """the pieces of one call in one device tensor, each at a 16-byte aligned start: (tensor, [device pointers])"""
    starts, pos = [], 0
    for p in pieces:
        starts.append(pos)
        pos = (pos + p.size + 15) & ~15
    buf = np.full(max(pos, 16), 0x5A, dtype=np.uint8)
    for s, p in zip(starts, pieces):
        buf[s:s + p.size] = p
    t = _dev(buf)
    return t, [t.data_ptr() + s for s in starts]


def md5_ios(d, fb, pieces, ptrs):
    ios = (d.FlacMd5IO * len(pieces))()
    for i, (p, ptr) in enumerate(zip(pieces, ptrs)):
        assert p.size % fb == 0
        ios[i].pcm, ios[i].frames = ptr, p.size // fb
    return ios


class Files:
    """n files' state records on the device, fresh from d2d_flac_md5_init_device unless `states` (bytes) is uploaded; update(pieces):
    one d2d_flac_md5_update_device call with one piece (a uint8 array, possibly empty) per file, and the same pieces through the
    host twin"""

    def __init__(self, d, channels, depth, n, states=None, stream=None):
        self.d, self.ch, self.depth, self.n, self.stream = d, channels, depth, n, stream
        self.fb = frame_bytes(channels, depth)
        self.keep = []
        if states is None:
            self.t_states = _dev(np.full(96 * n, 0xEE, dtype=np.uint8))
            d.flac_md5_init_device(self.t_states.data_ptr(), n, stream)
            self.host = d.flac_md5_init_host(n)
        else:
            self.t_states = _dev(np.frombuffer(states, dtype=np.uint8).copy())
            self.host = (d.FlacMd5State * n).from_buffer_copy(states)
        self.t_digests = _dev(np.full(16 * n, 0xEE, dtype=np.uint8))

    def update(self, pieces, first=0):
        """files first .. first + len(pieces) - 1"""
        t, ptrs = upload(pieces)
        self.keep.append(t)
        self.d.flac_md5_update_device(self.ch, self.depth, md5_ios(self.d, self.fb, pieces, ptrs), self.t_states.data_ptr() + 96 * first, self.stream)
        for i, p in enumerate(pieces):
            self.d.flac_md5_update_host(self.ch, self.depth, p, self.host[first + i])

    def records(self):
        r = _host(self.t_states).tobytes()
        return [r[96 * i:96 * i + 96] for i in range(self.n)]

    def host_records(self):
        return [record(s) for s in self.host]

    def digests(self):
        self.d.flac_md5_final_device(self.t_states.data_ptr(), self.n, self.t_digests.data_ptr(), self.stream)
        g = _host(self.t_digests).tobytes()
        return [g[16 * i:16 * i + 16] for i in range(self.n)]


def md5(pcm, depth):
    return hashlib.md5(hashed_bytes(pcm, depth)).digest()


@gpu
def test_every_residue_and_both_padding_cases(engine_lib):
    """files of 3 n bytes, n = 0 .. 130, mono 24-bit: every tail length 0 .. 63 at least twice, 183 = 2 * 64 + 55 (one padding block),
    120 = 64 + 56 (two), 192 (whole blocks), 0 (the empty message); as two calls of 128 and 3 files, then as one call of 131, which the
    library cuts into two launches"""
    rng = np.random.default_rng(3)
    pcms = [rng.integers(0, 256, 3 * n, dtype=np.uint8) for n in range(131)]
    want = [hashlib.md5(p.tobytes()).digest() for p in pcms]
    assert want[0].hex() == "d41d8cd98f00b204e9800998ecf8427e"
    two = Files(engine_lib, 1, 24, 131)
    two.update(pcms[:MAXF])
    two.update(pcms[MAXF:], first=MAXF)
    one = Files(engine_lib, 1, 24, 131)
    one.update(pcms)
    for f in (two, one):
        before = f.records()
        got = f.digests()
        assert [i for i in range(131) if got[i] != want[i]] == []
        assert f.records() == before == f.host_records()              # final does not modify the state
        assert f.digests() == got


@gpu
def test_seams_at_every_frame_of_a_short_message(engine_lib):
    """129 bytes (43 mono 24-bit frames) split in two calls at every frame 0 .. 43, 44 files in one pair of calls: after each call the 96
    bytes of every record are the host twin's.  A file fed as seven calls of 21 bytes: the first three leave 21, 42 and 63 bytes in the
    tail and complete no block"""
    d = engine_lib
    msg = np.random.default_rng(43).integers(0, 256, 129, dtype=np.uint8)
    f = Files(d, 1, 24, 44)
    assert f.records() == f.host_records()                             # init_device and init_host
    f.update([msg[:3 * s] for s in range(44)])
    assert f.records() == f.host_records()
    assert f.records()[0] == record(d.flac_md5_init_host(1)[0])       # frames == 0 left file 0's record as it was
    f.update([msg[3 * s:] for s in range(44)])
    assert f.records() == f.host_records()
    assert set(f.digests()) == {hashlib.md5(msg.tobytes()).digest()}
    seven = np.random.default_rng(7).integers(0, 256, 7 * 21, dtype=np.uint8)
    g = Files(d, 1, 24, 1)
    for k in range(7):
        g.update([seven[21 * k:21 * k + 21]])
        assert g.records() == g.host_records(), k
        assert g.host[0].tail_bytes == 21 * (k + 1) % 64
        assert g.digests()[0] == hashlib.md5(seven[:21 * k + 21].tobytes()).digest(), k
    assert d.lib().d2d_flac_md5_update_device(1, 24, None, 0, None, None) == 0          # n_files == 0 launches nothing


@gpu
@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("channels", CHANNELS)
def test_shapes_around_the_staging_size(engine_lib, channels, depth):
    """one frame under, at and one frame over S and 2 S (where a frame does not divide S: around the frame that straddles it), six files in
    one call; then each file continued by a second call of 5 frames, so that a seam follows a multi-trip call"""
    fb = frame_bytes(channels, depth)
    rng = np.random.default_rng(100 * channels + depth)
    lengths = [k * S // fb + e for k in (1, 2) for e in (-1, 0, 1)]
    pcms = []
    for n in lengths:
        p = rng.integers(0, 256, (n + 5) * fb, dtype=np.uint8)
        if depth == 20:                                               # full-scale negative samples: -2^19 and -1 in the container
            s = p.reshape(-1, 3)
            s[0::97] = (0x00, 0x00, 0x80)
            s[1::97] = (0xF0, 0xFF, 0xFF)
            s[-1] = (0x00, 0x00, 0x80)
        pcms.append(p)
    f = Files(engine_lib, channels, depth, len(lengths))
    f.update([p[:n * fb] for p, n in zip(pcms, lengths)])
    assert f.records() == f.host_records()
    assert f.digests() == [md5(p[:n * fb], depth) for p, n in zip(pcms, lengths)]
    f.update([p[n * fb:] for p, n in zip(pcms, lengths)])
    assert f.records() == f.host_records()
    assert f.digests() == [md5(p, depth) for p in pcms]
    assert min(lengths) * fb < S < (lengths[2]) * fb and lengths[3] * fb < 2 * S < lengths[5] * fb


@gpu
def test_bit_count_beyond_32_bits_from_a_state_built_by_hand(engine_lib):
    """a record with bytes = 2^29 - 3, arbitrary chaining values and its 61 tail bytes, continued by two mono 24-bit frames: 2^29 + 3 bytes,
    2^32 + 24 bits.  The digest is the host twin's from the same record (held to hashlib across that boundary by the CPU test)"""
    d = engine_lib
    rng = np.random.default_rng(61)
    st = d.FlacMd5State()
    st.h[:] = [int(v) for v in rng.integers(0, 1 << 32, 4, dtype=np.uint64)]
    st.bytes, st.tail_bytes, st.reserved = (1 << 29) - 3, 61, 0
    st.tail[:61] = [int(v) for v in rng.integers(0, 256, 61)]
    assert st.bytes % 64 == 61
    f = Files(d, 1, 24, 1, states=record(st))
    f.update([rng.integers(0, 256, 6, dtype=np.uint8)])
    assert f.host[0].bytes == (1 << 29) + 3 and f.host[0].tail_bytes == 3 and 8 * f.host[0].bytes >= 1 << 32
    assert f.records() == f.host_records()
    assert f.digests()[0] == d.flac_md5_final_host(f.host[0])
    low = d.FlacMd5State.from_buffer_copy(f.host_records()[0])          # (the same record with the count's bit 29 cleared hashes differently)
    low.bytes -= 1 << 29
    assert d.flac_md5_final_host(low) != f.digests()[0]


@gpu
@pytest.mark.parametrize("complement", (False, True))
def test_a_call_writes_only_the_records_or_only_the_digests(engine_lib, complement):
    """states, digests and pcm each in an arena between 32 KiB guards, two complementary fills: init and update change the state records
    only, final the digests only; a call refused for depth 17 or for a misaligned pcm changes no byte"""
    d, ch, depth = engine_lib, 2, 24
    fb = 6
    rng = np.random.default_rng(9)
    frames = (0, 1, 10, 11, S // fb + 3, 200)
    pcms = [rng.integers(0, 256, n * fb, dtype=np.uint8) for n in frames]
    n = len(frames)
    a_st, a_dg, a_in = Arena([96 * n]), Arena([16 * n]), Arena([p.size for p in pcms])
    fills = [fill_bytes(a.total, complement).copy() for a in (a_st, a_dg, a_in)]
    for s, p in zip(a_in.starts, pcms):
        fills[2][s:s + p.size] = p
    t_st, t_dg, t_in = (_dev(f) for f in fills)
    p_st, p_dg = t_st.data_ptr() + a_st.starts[0], t_dg.data_ptr() + a_dg.starts[0]

    def ios(misalign=None):
        x = (d.FlacMd5IO * n)()
        for i in range(n):
            x[i].pcm, x[i].frames = t_in.data_ptr() + a_in.starts[i] + (8 if misalign == i else 0), frames[i]
        return x

    def check(what, states, digests):
        for arena, t, fill, want in ((a_st, t_st, fills[0], states), (a_dg, t_dg, fills[1], digests)):
            v = violations(arena, _host(t), fill, [want])
            assert not v, what + ": " + describe(v)
        assert np.array_equal(_host(t_in), fills[2]), what + ": the pcm arena changed"

    host = d.flac_md5_init_host(n)
    as_bytes = lambda: np.frombuffer(b"".join(record(s) for s in host), dtype=np.uint8)
    d.flac_md5_init_device(p_st, n)
    check("init", as_bytes(), None)
    for bad_depth, misalign, text in ((17, None, "bit depth"), (24, 4, "16-byte aligned")):
        with pytest.raises(d.D2DError) as ei:
            d.flac_md5_update_device(ch, bad_depth, ios(misalign), p_st)
        assert ei.value.code == ERR_PARAM and text in ei.value.message
        check("refused: " + text, as_bytes(), None)
    with pytest.raises(d.D2DError) as ei:
        d.flac_md5_update_device(ch, depth, ios(), p_st + 8)
    assert ei.value.code == ERR_PARAM
    with pytest.raises(d.D2DError) as ei:
        d.flac_md5_final_device(p_st, n, 0)
    assert ei.value.code == ERR_PARAM
    check("refused: states and digests", as_bytes(), None)
    d.flac_md5_update_device(ch, depth, ios(), p_st)
    for i, p in enumerate(pcms):
        d.flac_md5_update_host(ch, depth, p, host[i])
    check("update", as_bytes(), None)
    d.flac_md5_final_device(p_st, n, p_dg)
    check("final", as_bytes(), np.frombuffer(b"".join(hashlib.md5(p.tobytes()).digest() for p in pcms), dtype=np.uint8))


def _engine_kw(channels, bit_depth):
    return dict(dsd_rate=1, output_rate=88200, channels=channels, fmt="I", endianness="M", block_size=1, filter="E",
                bit_depth=bit_depth, dither="T", seed=11)


def plain_pcm(d, kw, data, chunk):
    """the PCM d2d_convert_stream returns for `data` (bytes in the engine's layout) read in chunks of `chunk` bytes per channel"""
    pos, out = [0], []
    step = chunk * kw["channels"]

    def read(cap):
        a = pos[0]
        pos[0] = min(len(data), a + step)
        return data[a:pos[0]]

    e = d.Engine(**kw)
    e.convert_stream(read, out.append, total_bytes_per_channel=len(data) // kw["channels"], chunk_bytes_per_channel=chunk)
    e.close()
    return b"".join(out)


@gpu
def test_eight_updates_and_the_final_in_flight_behind_a_translate_call(engine_lib):
    """on a caller's non-blocking stream, with no wait between them: d2d_translate_batch_device makes the PCM, eight updates hash an eighth
    of its frames each (frames_out is known at return), final writes the digest; one synchronise"""
    import torch
    d, ch, depth = engine_lib, 2, 24
    kw = _engine_kw(ch, depth)
    nbytes = 4 * 6000 + 3
    chans = [synth("sine", nbytes, seed=31, msb_first=True), synth("pink", nbytes, seed=32, amp=0.098, msb_first=True)]
    data = pack_layout(chans, "I", 1)
    want_pcm = plain_pcm(d, kw, data.tobytes(), nbytes)
    e = d.Engine(**kw)
    fb = e.frame_bytes
    dsd = _dev(data)
    cap = e.next_frames(nbytes) + 64
    pcm = torch.zeros(cap * fb, dtype=torch.uint8, device="cuda")
    states = torch.zeros(96, dtype=torch.uint8, device="cuda")
    digest = torch.zeros(16, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    io = (d.FileIO * 1)()
    io[0].dsd, io[0].bytes_per_channel, io[0].pcm, io[0].pcm_capacity_bytes = dsd.data_ptr(), nbytes, pcm.data_ptr(), pcm.numel()
    d.flac_md5_init_device(states.data_ptr(), 1, s.cuda_stream)
    e.translate_batch_device(io, s.cuda_stream)
    nf = io[0].frames_out
    cuts = [nf * k // 8 // 8 * 8 for k in range(8)] + [nf]             # (a slice begins at a multiple of 8 frames: 48 bytes, 16-byte aligned)
    for a, b in zip(cuts[:-1], cuts[1:]):
        m = (d.FlacMd5IO * 1)()
        m[0].pcm, m[0].frames = pcm.data_ptr() + a * fb, b - a
        d.flac_md5_update_device(ch, depth, m, states.data_ptr(), s.cuda_stream)
    d.flac_md5_final_device(states.data_ptr(), 1, digest.data_ptr(), s.cuda_stream)
    s.synchronize()
    e.close()
    assert nf * fb == len(want_pcm) and nf > 8 * 64
    assert _host(pcm)[:nf * fb].tobytes() == want_pcm
    assert _host(digest).tobytes() == hashlib.md5(want_pcm).digest()


STREAM_BYTES = 4096 * 10            # per channel: 10240 frames at 88.2 kHz, two whole blocks and a short one
STREAM_CHUNK = 3 * 4096             # four chunks, the last a third of one


@pytest.fixture(scope="module")
def stream_input():
    chans = [synth("sine", STREAM_BYTES, seed=3, msb_first=True), synth("pink", STREAM_BYTES, seed=4, amp=0.098, msb_first=True)]
    return pack_layout(chans, "I", 1).tobytes()


@gpu
@pytest.mark.parametrize("check", (False, True), ids=("plain", "verified"))
@pytest.mark.parametrize("depth", DEPTHS)
def test_stream_driver_returns_the_md5_of_the_plain_conversion(engine_lib, stream_input, depth, check):
    d = engine_lib
    kw = _engine_kw(2, depth)
    want_pcm = np.frombuffer(plain_pcm(d, kw, stream_input, STREAM_CHUNK), dtype=np.uint8)

    def run(**how):
        pos, out = [0], []

        def read(cap):
            a = pos[0]
            pos[0] = min(len(stream_input), a + 2 * cap)
            return stream_input[a:pos[0]]

        e = d.Engine(**kw)
        r = e.convert_stream_flac(read, out.append, total_bytes_per_channel=STREAM_BYTES, chunk_bytes_per_channel=STREAM_CHUNK, effort=1, **how)
        e.close()
        return out, r

    plain, stats = run()
    hashed, r = run(md5=True, verify=check)
    mstats, digest = r[0], r[-1]
    assert digest == md5(want_pcm, depth)
    assert hashed == plain and len(plain) >= 3
    assert (mstats.samples_per_channel, mstats.blocks, mstats.min_frame_bytes, mstats.max_frame_bytes) == \
           (stats.samples_per_channel, stats.blocks, stats.min_frame_bytes, stats.max_frame_bytes)
    assert stats.samples_per_channel * frame_bytes(2, depth) == want_pcm.size and stats.blocks == 3 and stats.samples_per_channel % 4096
    if check:
        assert r[1].as_tuple() == (stats.samples_per_channel, stats.blocks, 0, d.FLAC_NO_BAD_BLOCK, d.FLAC_BAD_NONE)


@gpu
def test_stream_driver_on_an_empty_stream_and_on_failure(engine_lib):
    d = engine_lib
    e = d.Engine(**_engine_kw(2, 24))
    stats, digest = e.convert_stream_flac(lambda cap: b"", lambda b: None, md5=True)
    assert digest.hex() == "d41d8cd98f00b204e9800998ecf8427e" and stats.blocks == 0
    # a failure leaves md5 untouched: an unknown effort, and a null md5
    L, buf, st = d.lib(), (C.c_uint8 * 16)(*([0xEE] * 16)), d.FlacStreamStats()
    from dsd2dxd_amd._capi import PROGRESS_FN, READ_FN, WRITE_FN
    r, w, p = READ_FN(lambda u, dst, cap: 0), WRITE_FN(lambda u, q, n: 0), PROGRESS_FN(lambda u, pct: None)
    assert L.d2d_convert_stream_flac_md5(e._h, 24, 7, r, None, w, None, None, p, None, 0, 0, C.byref(st), None, buf) == ERR_PARAM
    assert bytes(buf) == bytes([0xEE] * 16)
    assert L.d2d_convert_stream_flac_md5(e._h, 24, 0, r, None, w, None, None, p, None, 0, 0, C.byref(st), None, None) == ERR_PARAM
    e.close()


@gpu
@pytest.mark.parametrize("effort", (0, 12))
def test_cli_flac_md5_writes_the_host_sinks_file(engine_lib, tmp_path, effort):
    if not os.path.exists(CLI):
        engine_lib.build_library()
    n = 4096 * 6 + 500
    chans = [synth("sine", n, seed=7), synth("pink", n, seed=8, amp=0.098)]
    for name in ("host", "gpu", "hashed"):
        (tmp_path / name).mkdir()
        write_dsf(str(tmp_path / name / "y.dsf"), chans)
    args = [CLI, "convert", "-o", "f", "-r", "88200", "-b", "24", "-d", "T", "-q", "--flac-effort", str(effort)]
    subprocess.check_call(args + [str(tmp_path / "host" / "y.dsf")])
    subprocess.check_call(args + ["--gpu-flac", str(tmp_path / "gpu" / "y.dsf")])
    subprocess.check_call(args + ["--gpu-flac", "--flac-md5"] + (["--flac-verify"] if effort else []) + [str(tmp_path / "hashed" / "y.dsf")])
    h, g, m = ((tmp_path / k / "y.flac").read_bytes() for k in ("host", "gpu", "hashed"))
    assert m == h                                                      # equal in every byte
    assert g[26:42] == bytes(16) and g[:26] == h[:26] and g[42:] == h[42:] and h[26:42] != bytes(16)
    r = subprocess.run([CLI, "verify", str(tmp_path / "hashed" / "y.flac"), str(tmp_path / "gpu" / "y.flac")], capture_output=True, text=True)
    lines = r.stdout.splitlines()
    assert r.returncode == 0 and lines[0].endswith(": ok") and lines[1].endswith(": ok (no MD5 in STREAMINFO)"), (r.stdout, r.stderr)
