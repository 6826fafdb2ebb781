"""FLAC frames on the GPU (include/dsd2dxd_amd.h): d2d_flac_encode_device, d2d_convert_stream_flac and the CLI's --gpu-flac against
d2d_flac_encode_host -- the sink's own encoder, pinned to the format by tests/test_flac_cpu.py -- byte for byte, and against the
subset decoder of flac_ref.py.  Every call's buffers are small; the shape matrix sends the eight lengths of a (channels, depth,
signal) cell through ONE call as eight files, so the whole matrix is sixty launches."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import flac_ref as R
from helpers import pack_layout, synth, write_dsf
from test_flac_cpu import BOUNDARIES, CHANNELS, DEPTHS, LENGTHS
from test_gpu_containment import Arena, describe, fill_bytes, violations

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "dsd2dxd_amd", "dsd2dxd_amd_cli")


def _dev(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    assert t.data_ptr() % 16 == 0
    return t


def _host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


def host_encode(d, channels, depth, files):
    """files: [(pcm uint8 array, first_block, final)] -> [(frame bytes, (bytes_out, min, max), frames consumed)]"""
    out = []
    for pcm, first, final in files:
        b, res, used = d.flac_encode_host(channels, depth, pcm, first_block=first, final=final)
        out.append((b, (res.bytes_out, res.min_frame_bytes, res.max_frame_bytes), used))
    return out


def device_encode(d, channels, depth, files, slack=0):
    """one d2d_flac_encode_device call over `files`, each in buffers of its own; the same shape of result as host_encode, plus blocks"""
    fb = channels * (2 if depth == 16 else 3)
    n = len(files)
    ios = (d.FlacIO * n)()
    keep, ws = [], 0
    rec = _dev(np.full(16 * n, 0xEE, dtype=np.uint8))
    for i, (pcm, first, final) in enumerate(files):
        frames = pcm.size // fb
        cap = d.flac_bound_bytes(channels, depth, frames, final)
        tp, to = _dev(pcm), _dev(np.full(cap + slack, 0xA5, dtype=np.uint8))
        keep.append((tp, to))
        ios[i].pcm, ios[i].frames, ios[i].first_block, ios[i].final = tp.data_ptr(), frames, first, int(final)
        ios[i].out, ios[i].out_capacity_bytes, ios[i].result = to.data_ptr(), cap, rec.data_ptr() + 16 * i
        ws += d.flac_workspace_bytes(channels, depth, frames, final)
    tw = _dev(np.zeros(max(ws, 16), dtype=np.uint8))
    d.flac_encode_device(channels, depth, ios, tw.data_ptr(), ws)
    r = _host(rec).view(np.uint64).reshape(n, 2)
    got = []
    for i in range(n):
        bytes_out, mm = int(r[i, 0]), int(r[i, 1])
        o = _host(keep[i][1])
        assert (o[bytes_out:] == 0xA5).all(), f"file {i}: bytes behind bytes_out were written"
        got.append((o[:bytes_out].tobytes(), (bytes_out, mm & 0xFFFFFFFF, mm >> 32), ios[i].frames_consumed, ios[i].blocks))
    return got


def _blocks(frames, final):
    return frames // 4096 + (1 if final and frames % 4096 else 0)


@gpu
@pytest.mark.parametrize("signal", R.SIGNALS)
@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("channels", CHANNELS)
def test_shape_matrix_equals_the_host_encoder(engine_lib, channels, depth, signal):
    files = []
    for i, (frames, final) in enumerate(LENGTHS):
        s = R.signal(signal, frames, channels, depth, seed=frames + channels)
        files.append((R.pack_pcm(s, depth), 5 + 100 * i, final))
    want = host_encode(engine_lib, channels, depth, files)
    got = device_encode(engine_lib, channels, depth, files)
    for i, (g, w) in enumerate(zip(got, want)):
        what = f"file {i}: {LENGTHS[i]}"
        assert g[1] == w[1], what                                  # the result record
        assert g[0] == w[0], what                                  # the frames
        assert g[2] == w[2] and g[3] == _blocks(*LENGTHS[i]), what  # frames_consumed, blocks


@gpu
def test_frame_numbers_across_utf8_lengths_on_the_device(engine_lib):
    firsts = list(BOUNDARIES) + [(1 << 31) - 2]                   # ... and the last legal number
    files = [(R.pack_pcm(R.signal("random", 2 * 4096, 1, 16, seed=f), 16), f, True) for f in firsts]
    want = host_encode(engine_lib, 1, 16, files)
    got = device_encode(engine_lib, 1, 16, files)
    for g, w, f in zip(got, want, firsts):
        assert g[:3] == w, hex(f)
        back, _ = R.decode(g[0], 1, 16, first_block=f)
        assert back.shape[0] == 2 * 4096
    with pytest.raises(engine_lib.D2DError) as ei:                # one beyond: refused on the host
        device_encode(engine_lib, 1, 16, [(files[0][0], (1 << 31) - 1, True)])
    assert ei.value.code == -1 and "31 bits" in ei.value.message


RAGGED = ((0, False, 9), (1000, False, 0), (4096, False, 0x7F), (3 * 4096 + 17, True, 1000), (2 * 4096, False, 77))


@gpu
def test_ragged_batch_and_determinism(engine_lib):
    files = [(R.pack_pcm(R.signal("sine" if i % 2 else "random", n, 2, 24, seed=i), 24), first, final) for i, (n, final, first) in enumerate(RAGGED)]
    want = host_encode(engine_lib, 2, 24, files)
    got = device_encode(engine_lib, 2, 24, files)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g[:3] == w and g[3] == _blocks(RAGGED[i][0], RAGGED[i][1]), i
    assert [g[3] for g in got] == [0, 0, 1, 4, 2] and got[0][1] == (0, 0, 0) and got[1][1] == (0, 0, 0)
    assert device_encode(engine_lib, 2, 24, files) == got          # the same call again: the same bytes
    # more files than one launch carries descriptors for (16): every file still gets its own frames
    many = [files[2 + i % 3] for i in range(19)]
    again = device_encode(engine_lib, 2, 24, many)
    assert [g[:3] for g in again] == [want[2 + i % 3] for i in range(19)]


@gpu
@pytest.mark.parametrize("complement", (False, True))
def test_a_call_writes_only_what_it_reports(engine_lib, complement):
    """out buffers back to back with exact capacities, the workspace and the result records between guards, two complementary fills: after
    a successful call only [0, bytes_out) of each out, the records and the inside of the workspace differ from the fill; after a refused
    call nothing does"""
    d, ch, depth = engine_lib, 3, 24
    fb = ch * 3
    shapes = ((4096 + 5, True, 3), (0, True, 0), (2 * 4096 + 100, False, 0x7FF), (4096, True, 1))
    pcms = [R.pack_pcm(R.signal("sine" if i % 2 else "random", n, ch, depth, seed=i), depth) for i, (n, _, _) in enumerate(shapes)]
    caps = [d.flac_bound_bytes(ch, depth, n, f) for n, f, _ in shapes]
    wss = sum(d.flac_workspace_bytes(ch, depth, n, f) for n, f, _ in shapes)
    a_in, a_out, a_ws, a_rec = Arena([p.size for p in pcms]), Arena(caps), Arena([wss]), Arena([16 * len(shapes)])
    fills = [fill_bytes(a.total, complement).copy() for a in (a_in, a_out, a_ws, a_rec)]
    for s, p in zip(a_in.starts, pcms):
        fills[0][s:s + p.size] = p
    t_in, t_out, t_ws, t_rec = (_dev(f) for f in fills)

    def ios(short=None):
        x = (d.FlacIO * len(shapes))()
        for i, (n, final, first) in enumerate(shapes):
            x[i].pcm, x[i].frames, x[i].first_block, x[i].final = t_in.data_ptr() + a_in.starts[i], n, first, int(final)
            x[i].out, x[i].out_capacity_bytes = t_out.data_ptr() + a_out.starts[i], caps[i] - (1 if short == i else 0)
            x[i].result = t_rec.data_ptr() + a_rec.starts[0] + 16 * i
        return x

    def unchanged(what):
        for t, f, name in ((t_in, fills[0], "pcm"), (t_out, fills[1], "out"), (t_ws, fills[2], "workspace"), (t_rec, fills[3], "records")):
            assert np.array_equal(_host(t), f), f"{what}: the {name} arena changed"

    # refused: one file's capacity a byte short; a workspace a byte short
    with pytest.raises(d.D2DError) as ei:
        d.flac_encode_device(ch, depth, ios(short=2), t_ws.data_ptr() + a_ws.starts[0], wss)
    assert ei.value.code == -20
    unchanged("capacity one byte short")
    with pytest.raises(d.D2DError) as ei:
        d.flac_encode_device(ch, depth, ios(), t_ws.data_ptr() + a_ws.starts[0], wss - 1)
    assert ei.value.code == -20
    unchanged("workspace one byte short")

    want = host_encode(d, ch, depth, [(p, first, final) for p, (_, final, first) in zip(pcms, shapes)])
    d.flac_encode_device(ch, depth, ios(), t_ws.data_ptr() + a_ws.starts[0], wss)
    got_out, got_ws, got_rec = _host(t_out), _host(t_ws), _host(t_rec)
    expect = []
    for i, (b, _, _) in enumerate(want):
        w = fills[1][a_out.starts[i]:a_out.end(i)].copy()
        w[:len(b)] = np.frombuffer(b, dtype=np.uint8)
        expect.append(w if caps[i] else None)
    v = violations(a_out, got_out, fills[1], expect)
    assert not v, describe(v)
    v = violations(a_ws, got_ws, fills[2], [got_ws[a_ws.starts[0]:a_ws.end(0)]])       # the inside is the call's own
    assert not v, "workspace: " + describe(v)
    rec = np.zeros(len(shapes) * 2, dtype=np.uint64)
    for i, (_, r, _) in enumerate(want):
        rec[2 * i], rec[2 * i + 1] = r[0], r[1] | (r[2] << 32)
    v = violations(a_rec, got_rec, fills[3], [rec.view(np.uint8)])
    assert not v, "records: " + describe(v)
    assert np.array_equal(_host(t_in), fills[0]), "the pcm arena changed"


CHAINED = (dict(channels=2, bit_depth=24), dict(channels=3, bit_depth=16), dict(channels=2, bit_depth=20))


def _engine_kw(channels, bit_depth):
    return dict(dsd_rate=1, output_rate=88200, channels=channels, fmt="I", endianness="M", block_size=1, filter="E",
                bit_depth=bit_depth, dither="T", seed=11)


@gpu
@pytest.mark.parametrize("shape", CHAINED, ids=lambda s: f"{s['channels']}ch{s['bit_depth']}")
def test_chained_with_the_engine(engine_lib, oracle_mod, shape):
    """three ragged translate calls write behind the carried remainder, each followed by the encode call on the same stream, `final` on
    the last: the concatenated frames are the host encoding of the oracle's PCM for the whole stream"""
    import torch
    d, ch, depth = engine_lib, shape["channels"], shape["bit_depth"]
    kw = _engine_kw(ch, depth)
    lens = (4 * 5000 + 1, 4 * 1500 + 2, 4 * (2 * 4096 + 777 - 6500) + 1)          # bytes per channel of the three calls
    total = sum(lens)
    chans = [synth("sine" if c % 2 == 0 else "pink", total, seed=20 + c, amp=0.352 if c % 2 == 0 else 0.098, msb_first=True) for c in range(ch)]
    ref, rf = oracle_mod.Oracle(**kw).translate(pack_layout(chans, "I", 1))
    e = d.Engine(**kw)
    fb = e.frame_bytes
    ref = ref[:rf * fb]
    assert rf > 2 * 4096 and rf % 4096
    cap_frames = rf + 64
    pcm = torch.zeros(cap_frames * fb, dtype=torch.uint8, device="cuda")
    tmp = torch.zeros(cap_frames * fb, dtype=torch.uint8, device="cuda")
    out = torch.zeros(d.flac_bound_bytes(ch, depth, cap_frames, 1), dtype=torch.uint8, device="cuda")
    ws = torch.zeros(d.flac_workspace_bytes(ch, depth, cap_frames, 1), dtype=torch.uint8, device="cuda")
    rec = torch.zeros(16, dtype=torch.uint8, device="cuda")
    frames_out, carry, block, at = [], 0, 0, 0
    for call, n in enumerate(lens):
        dsd = _dev(pack_layout([c[at:at + n] for c in chans], "I", 1))
        at += n
        io = (d.FileIO * 1)()
        io[0].dsd, io[0].bytes_per_channel, io[0].pcm, io[0].pcm_capacity_bytes = dsd.data_ptr(), n, tmp.data_ptr(), tmp.numel()
        e.translate_batch_device(io)
        nf = io[0].frames_out
        # (the translate call wants a 16-byte aligned pcm, the end of the carry has no alignment: its frames go behind the carry by a copy)
        pcm[carry * fb:(carry + nf) * fb] = tmp[:nf * fb]
        f = (d.FlacIO * 1)()
        f[0].pcm, f[0].frames, f[0].first_block, f[0].final = pcm.data_ptr(), carry + nf, block, int(call == len(lens) - 1)
        f[0].out, f[0].out_capacity_bytes, f[0].result = out.data_ptr(), out.numel(), rec.data_ptr()
        d.flac_encode_device(ch, depth, f, ws.data_ptr(), ws.numel())
        bytes_out = int(_host(rec).view(np.uint64)[0])
        frames_out.append(_host(out)[:bytes_out].tobytes())
        block += f[0].blocks
        rest = f[0].frames - f[0].frames_consumed
        assert rest < 4096 and (rest == 0 or call < len(lens) - 1)
        if rest and f[0].frames_consumed:
            pcm[:rest * fb] = pcm[f[0].frames_consumed * fb:(f[0].frames_consumed + rest) * fb].clone()
        carry = rest
    e.close()
    got = b"".join(frames_out)
    want, res, used = d.flac_encode_host(ch, depth, ref, first_block=0, final=True)
    assert used == rf and got == want
    back, sizes = R.decode(got, ch, depth)
    assert np.array_equal(back, R.unpack_pcm(ref, ch, depth)) and len(sizes) == block == 3


STREAM_KW = dict(dsd_rate=1, output_rate=88200, channels=2, fmt="P", endianness="L", block_size=4096, filter="E", bit_depth=24, dither="T", seed=5)


@gpu
def test_whole_stream_twin(engine_lib, oracle_mod):
    """d2d_convert_stream_flac with chunks of 3072 frames: blocks straddle chunks, the last block is short"""
    d = engine_lib
    nbytes = 4096 * 10
    chans = [synth("sine", nbytes, seed=3), synth("pink", nbytes, seed=4, amp=0.098)]
    chunk = 3 * 4096
    pos = [0]

    def read(cap):
        assert cap == chunk
        a = pos[0]
        b = min(nbytes, a + cap)
        pos[0] = b
        return pack_layout([c[a:b] for c in chans], "P", 4096).tobytes() if b > a else b""

    ref, rf = oracle_mod.Oracle(**STREAM_KW).translate(pack_layout(chans, "P", 4096))
    want, res, _ = d.flac_encode_host(2, 24, ref[:rf * 6], first_block=0, final=True)
    out, prog = [], []
    e = d.Engine(**STREAM_KW)
    stats = e.convert_stream_flac(read, out.append, total_bytes_per_channel=nbytes, chunk_bytes_per_channel=chunk, progress=prog.append)
    assert b"".join(out) == want
    assert (stats.samples_per_channel, stats.blocks, stats.min_frame_bytes, stats.max_frame_bytes) == \
           (rf, rf // 4096 + 1, res.min_frame_bytes, res.max_frame_bytes)
    assert rf % 4096 and rf > 2 * 4096
    assert all(o[:2] == b"\xff\xf8" for o in out)                  # every write begins with a frame
    assert prog[-1] == 100.0 and all(p < 100.0 for p in prog[:-1]) and prog == sorted(prog)
    assert np.array_equal(R.decode(want, 2, 24)[0], R.unpack_pcm(ref[:rf * 6], 2, 24))
    e.close()
    # cancel: polled between chunks
    pos[0] = 0
    flag, seen = C.c_int(0), []

    def write_then_cancel(b):
        seen.append(len(b))
        flag.value = 1

    e2 = d.Engine(**STREAM_KW)
    with pytest.raises(d.D2DError) as ei:
        e2.convert_stream_flac(read, write_then_cancel, total_bytes_per_channel=nbytes, chunk_bytes_per_channel=chunk, cancel=flag)
    assert ei.value.code == -30 and len(seen) == 1
    e2.close()


@gpu
def test_cli_gpu_flac_equals_the_host_sink_except_md5(engine_lib, oracle_mod, tmp_path):
    from test_host_driver import make_id3
    if not os.path.exists(CLI):
        engine_lib.build_library()
    n = 4096 * 6 + 500
    chans = [synth("sine", n, seed=7), synth("pink", n, seed=8, amp=0.098)]
    tag = make_id3(3, [(b"TIT2", b"\x00A title"), (b"TPE1", b"\x00An artist")])
    for name in ("host", "gpu"):
        (tmp_path / name).mkdir()
        write_dsf(str(tmp_path / name / "y.dsf"), chans, id3=tag)
    args = [CLI, "convert", "-o", "f", "-r", "88200", "-b", "24", "-d", "T", "-q"]
    subprocess.check_call(args + [str(tmp_path / "host" / "y.dsf")])
    subprocess.check_call(args + ["--gpu-flac", str(tmp_path / "gpu" / "y.dsf")])
    h, g = (tmp_path / "host" / "y.flac").read_bytes(), (tmp_path / "gpu" / "y.flac").read_bytes()
    assert len(h) == len(g) and h[:26] == g[:26] and h[42:] == g[42:]
    assert g[26:42] == bytes(16) and h[26:42] != bytes(16)          # STREAMINFO's MD5: "not computed" on the GPU path
    assert b"A title" in g[:4096]
    # the audio of the GPU file, decoded, is the oracle's
    pos, last = 4, False
    while not last:
        last, blen = bool(g[pos] & 0x80), int.from_bytes(g[pos + 1:pos + 4], "big")
        pos += 4 + blen
    kw = dict(dsd_rate=1, output_rate=88200, channels=2, fmt="P", endianness="L", block_size=4096, bit_depth=24, dither="T", seed=0)
    ref, rf = oracle_mod.Oracle(**kw).translate(pack_layout(chans, "P", 4096))
    back, sizes = R.decode(g[pos:], 2, 24)
    assert rf == n * 8 // 32 and np.array_equal(back, R.unpack_pcm(ref[:rf * 6], 2, 24))
    si = g[8:42]
    assert int.from_bytes(si[4:7], "big") == min(sizes) and int.from_bytes(si[7:10], "big") == max(sizes)
    assert int.from_bytes(si[10:18], "big") & ((1 << 36) - 1) == rf
    # any other output type ignores the switch
    subprocess.check_call([CLI, "convert", "-o", "w", "-r", "88200", "-b", "24", "-d", "T", "-q", "--gpu-flac", str(tmp_path / "gpu" / "y.dsf")])
    subprocess.check_call([CLI, "convert", "-o", "w", "-r", "88200", "-b", "24", "-d", "T", "-q", str(tmp_path / "host" / "y.dsf")])
    assert (tmp_path / "gpu" / "y.wav").read_bytes() == (tmp_path / "host" / "y.wav").read_bytes()
