"""Loudness on the GPU (include/dsd2dxd_amd.h, "Loudness where the PCM is": d2d_loud_measure_device, the stream driver
d2d_convert_stream_flac_loud, the CLI's --replaygain and `levels --loudness`).  The reference of every cell is the host twin,
d2d_loud_measure_host, which compiles the same loud_meter.h and which tests/test_loudness_cpu.py holds to an independent numpy / scipy
restatement: device cells must be the twin's BYTES, no tolerance.  Rate 8000 makes a sub-block 800 frames; every call measures a few
thousand frames per file."""
import os
import re
import subprocess

import numpy as np
import pytest

import loudness_ref as R
from helpers import pack_layout, synth, write_dsf
from test_gpu_containment import Arena, describe, fill_bytes, violations
from test_gpu_flac_md5 import _dev, _engine_kw, _host, plain_pcm, upload
from test_loudness_cpu import noise_pcm, vorbis_fields

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "dsd2dxd_amd", "dsd2dxd_amd_cli")
ERR_PARAM, ERR_CAPACITY = -1, -20
MAXF = 64           # the files of one launch: MAXF in dsd2dxd_amd/csrc/loud/d2d_loud.hip
SLACK = 3           # cells of capacity behind what a call writes: they must stay as they were
EE = np.frombuffer(bytes([0xEE] * 8), dtype=np.float64)[0]


def twin(d, ch, depth, rate, piece, first_frame, first_subblock, final):
    """the host twin's cells of one file as bytes, and its counts (frames == 0: no cells, the counts a caller's record keeps)"""
    if piece.size == 0:
        return b"", (None, 0, None)
    cells, io = d.loud_measure_host(ch, depth, rate, piece, first_frame=first_frame, first_subblock=first_subblock, final=final)
    return cells.tobytes(), (io.subblocks, io.cells_out, io.next_subblock)


def device_call(d, ch, depth, rate, pieces, firsts=None, subs=None, final=True, stream=None):
    """one d2d_loud_measure_device call with one piece per file; returns per file (cell bytes written, counts) after checking that the
    capacity behind cells_out was left alone"""
    n = len(pieces)
    firsts, subs = firsts or [0] * n, subs or [0] * n
    want = [twin(d, ch, depth, rate, p, firsts[i], subs[i], final) for i, p in enumerate(pieces)]
    caps = [w[1][1] + SLACK for w in want]
    starts = np.concatenate([[0], np.cumsum(caps)]).astype(int)
    t_cells = _dev(np.full(2 * int(starts[-1]), EE, dtype=np.float64))
    t_pcm, ptrs = upload(pieces)
    ios = (d.LoudIO * n)()
    for i in range(n):
        fb = ch * R.sample_bytes(depth)
        ios[i] = d.LoudIO(ptrs[i], pieces[i].size // fb, firsts[i], subs[i], int(final), 0, t_cells.data_ptr() + 16 * int(starts[i]), caps[i], 111, 222, 333)
    d.loud_measure_device(ch, depth, rate, ios, stream)
    got = _host(t_cells).reshape(-1, 2)
    out = []
    for i in range(n):
        if pieces[i].size == 0:                                            # left alone, the counts too
            assert (ios[i].subblocks, ios[i].cells_out, ios[i].next_subblock) == (111, 222, 333)
            k = 0
        else:
            assert (ios[i].subblocks, ios[i].cells_out, ios[i].next_subblock) == want[i][1], (i, want[i][1])
            k = ios[i].cells_out
        region = got[starts[i]:starts[i + 1]]
        assert region[k:].tobytes() == bytes([0xEE]) * (16 * (caps[i] - k)), f"file {i}: cells behind cells_out were written"
        out.append(region[:k].tobytes())
    return out, want


@gpu
@pytest.mark.parametrize("depth", (16, 20, 24, 32))
@pytest.mark.parametrize("channels", (1, 2, 3, 6, 8))
def test_device_cells_are_the_host_twins_bytes(engine_lib, channels, depth):
    """four files in one call -- 0 frames, under one sub-block, exactly 3 sub-blocks, 7 sub-blocks and a partial -- final and not"""
    rate, S = 8000, 800
    pieces = [noise_pcm(n, channels, depth, seed=10 * channels + k) if n else np.zeros(0, dtype=np.uint8)
              for k, n in enumerate((0, 300, 3 * S, 7 * S + 123))]
    for final in (True, False):
        got, want = device_call(engine_lib, channels, depth, rate, pieces, final=final)
        rows = [len(g) // (16 * channels) for g in got]
        assert rows == ([0, 1, 3, 8] if final else [0, 0, 3, 7])
        for i in range(4):
            assert got[i] == want[i][0], f"file {i}, final {final}: the device cells are not the host twin's bytes"


@gpu
def test_stereo_24_bit_at_88200(engine_lib):
    rate, S = 88200, 8820
    piece = noise_pcm(5 * S, 2, 24, seed=88)
    got, want = device_call(engine_lib, 2, 24, rate, [piece])
    assert len(got[0]) == 5 * 2 * 16 and got[0] == want[0][0]
    ref = R.cells(R.to_float(piece, 2, 24), rate)                          # ... and the twin is the reference's, here too
    cells = np.frombuffer(got[0], dtype=np.float64).reshape(5, 2, 2)
    assert np.max(np.abs(cells[:, :, 0] - ref[:, :, 0]) / ref[:, :, 0]) <= 1e-10 and np.array_equal(cells[:, :, 1], ref[:, :, 1])


@gpu
def test_more_files_than_one_launch_holds(engine_lib):
    """2 * MAXF + 3 mono 16-bit files of different lengths, some empty, in one call: the library cuts it into three launches"""
    S = 800
    pieces = [noise_pcm(S + 37 * k, 1, 16, seed=k) if k % 9 else np.zeros(0, dtype=np.uint8) for k in range(2 * MAXF + 3)]
    got, want = device_call(engine_lib, 1, 16, 8000, pieces)
    assert [i for i in range(len(pieces)) if got[i] != want[i][0]] == []
    assert sum(len(g) for g in got) // 16 > 3 * (2 * MAXF + 3)


@gpu
@pytest.mark.parametrize("channels,depth", [(2, 24), (3, 16), (1, 32)])
def test_a_stream_cut_into_calls_with_the_minimum_preroll(engine_lib, channels, depth):
    """one call per sub-block, each with PCM from frame max(0, j - 2) * S and nothing more in front (sub-blocks 0 and 1: the clamped
    pre-roll); then ragged cuts; the cells are those of the whole stream in one call"""
    d, rate, S = engine_lib, 8000, 800
    frames = 6 * S + 55
    pcm = noise_pcm(frames, channels, depth, seed=21)
    fb = channels * R.sample_bytes(depth)
    whole, _ = twin(d, channels, depth, rate, pcm, 0, 0, True)
    for ends in ([S * k for k in range(1, 7)] + [frames], [S // 2, S + 3, 4 * S - 1, 4 * S, frames]):
        got, nxt = b"", 0
        for end in ends:
            first = max(0, nxt - 2) * S
            (cells,), want = device_call(d, channels, depth, rate, [pcm[first * fb:end * fb]], [first], [nxt], final=end == frames)
            assert cells == want[0][0]
            got += cells
            nxt = end // S
        assert got == whole, ends


@gpu
@pytest.mark.parametrize("complement", (False, True))
def test_a_call_writes_its_cells_and_reads_its_frames(engine_lib, complement):
    """pcm and cells each in an arena between 32 KiB guards, files back to back, capacities exact, two complementary fills: exactly
    cells_out cells per file are written and they are the twin's whatever lies behind the declared frames; refused calls change no byte"""
    d, ch, depth, rate, S = engine_lib, 3, 24, 8000, 800
    frames = (2 * S + 1, 0, 5, 4 * S, 3 * S + 799)
    firsts, subs = (0, 0, 0, 0, 0), (0, 0, 0, 1, 2)
    pcms = [noise_pcm(n, ch, depth, seed=40 + i) if n else np.zeros(0, dtype=np.uint8) for i, n in enumerate(frames)]
    n = len(frames)
    want = [twin(d, ch, depth, rate, pcms[i], firsts[i], subs[i], True) for i in range(n)]
    a_in, a_out = Arena([p.size for p in pcms]), Arena([len(w[0]) for w in want])
    f_in, f_out = fill_bytes(a_in.total, complement).copy(), fill_bytes(a_out.total, complement).copy()
    for s, p in zip(a_in.starts, pcms):
        f_in[s:s + p.size] = p
    t_in, t_out = _dev(f_in), _dev(f_out)

    def ios(change=None):
        x = (d.LoudIO * n)()
        for i in range(n):
            x[i] = d.LoudIO(t_in.data_ptr() + a_in.starts[i], frames[i], firsts[i], subs[i], 1, 0, t_out.data_ptr() + a_out.starts[i], len(want[i][0]) // 16, 111, 222, 333)
        for (i, field), v in (change or {}).items():
            setattr(x[i], field, getattr(x[i], field) + v)
        return x

    def check(what, cells):
        v = violations(a_out, _host(t_out), f_out, cells)
        assert not v, what + ": " + describe(v)
        assert np.array_equal(_host(t_in), f_in), what + ": the pcm arena changed"

    refusals = [((ch, 17, rate), {}, ERR_PARAM, "bit depth"), ((9, depth, rate), {}, ERR_PARAM, "channel"), ((ch, depth, 8004), {}, ERR_PARAM, "rate"),
                ((ch, depth, rate), {(3, "pcm"): 8}, ERR_PARAM, "aligned"), ((ch, depth, rate), {(0, "cells"): 8}, ERR_PARAM, "aligned"),
                ((ch, depth, rate), {(4, "first_frame"): 1}, ERR_PARAM, "pre-roll"), ((ch, depth, rate), {(4, "first_subblock"): 1, (4, "first_frame"): S + 1}, ERR_PARAM, "pre-roll"),
                ((ch, depth, rate), {(4, "cells_capacity"): -1}, ERR_CAPACITY, "cells_capacity")]
    for args, kw, code, text in refusals:
        x = ios(kw)
        with pytest.raises(d.D2DError) as ei:
            d.loud_measure_device(*args, x)
        assert ei.value.code == code and text in ei.value.message, (args, kw, ei.value)
        assert all((x[i].subblocks, x[i].cells_out, x[i].next_subblock) == (111, 222, 333) for i in range(n)), "a refused call wrote counts"
        check("refused: " + text, [None] * n)
    x = ios()
    d.loud_measure_device(ch, depth, rate, x)
    assert [x[i].cells_out for i in range(n)] == [9, 222, 3, 9, 6]
    check("measured", [np.frombuffer(w[0], dtype=np.uint8) if w[0] else None for w in want])
    d.loud_measure_device(ch, depth, rate, (d.LoudIO * 0)())               # n_files == 0: nothing
    check("no files", [np.frombuffer(w[0], dtype=np.uint8) if w[0] else None for w in want])


@gpu
def test_measured_in_flight_behind_a_translate_call(engine_lib):
    """on a caller's non-blocking stream, with no wait between them: d2d_translate_batch_device makes 88.2 kHz PCM and the measure call
    takes it where it lies (frames_out is known at return); one synchronise; against the host twin on the downloaded frames"""
    import torch
    d, ch, depth, rate = engine_lib, 2, 24, 88200
    kw = _engine_kw(ch, depth)
    nbytes = 4 * 8820 * 3 + 4 * 3000                                       # 4 bytes per channel make a frame: 3 sub-blocks and a partial one
    chans = [synth("sine", nbytes, seed=31, msb_first=True), synth("pink", nbytes, seed=32, amp=0.098, msb_first=True)]
    data = pack_layout(chans, "I", 1)
    e = d.Engine(**kw)
    fb = e.frame_bytes
    dsd = _dev(data)
    cap = e.next_frames(nbytes) + 64
    pcm = torch.zeros(cap * fb, dtype=torch.uint8, device="cuda")
    cells = _dev(np.full(2 * 16, EE, dtype=np.float64))
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    io = (d.FileIO * 1)()
    io[0].dsd, io[0].bytes_per_channel, io[0].pcm, io[0].pcm_capacity_bytes = dsd.data_ptr(), nbytes, pcm.data_ptr(), pcm.numel()
    e.translate_batch_device(io, s.cuda_stream)
    nf = io[0].frames_out
    lio = (d.LoudIO * 1)()
    lio[0] = d.LoudIO(pcm.data_ptr(), nf, 0, 0, 1, 0, cells.data_ptr(), 16, 0, 0, 0)
    d.loud_measure_device(ch, depth, rate, lio, s.cuda_stream)
    s.synchronize()
    e.close()
    frames = _host(pcm)[:nf * fb]
    want, counts = twin(d, ch, depth, rate, frames, 0, 0, True)
    assert nf // 8820 == 3 and nf % 8820 and (lio[0].subblocks, lio[0].cells_out, lio[0].next_subblock) == counts == (3, 8, 3)
    assert _host(cells).tobytes()[:len(want)] == want and frames.any()


STREAM_BYTES = 4096 * 48            # per channel: 49152 frames at 88.2 kHz, 5 sub-blocks and a partial one, 12 FLAC blocks
STREAM_CHUNK = 5 * 4096             # ten chunks, the last three fifths of one


@gpu
@pytest.mark.parametrize("md5,check", [(False, False), (True, True)], ids=("plain", "hashed-verified"))
def test_stream_driver_feeds_the_meter(engine_lib, md5, check):
    """d2d_convert_stream_flac_loud: the frames and stats of the call without the meter, and a meter that finishes with the bytes the host
    twin and the same integration give on the plain conversion's PCM"""
    d, ch, depth, rate = engine_lib, 2, 24, 88200
    kw = _engine_kw(ch, depth)
    chans = [synth("sine", STREAM_BYTES, seed=3, msb_first=True), synth("pink", STREAM_BYTES, seed=4, amp=0.098, msb_first=True)]
    data = pack_layout(chans, "I", 1).tobytes()
    want_pcm = np.frombuffer(plain_pcm(d, kw, data, STREAM_CHUNK), dtype=np.uint8)

    def run(**how):
        pos, out = [0], []

        def read(cap):
            a = pos[0]
            pos[0] = min(len(data), a + 2 * cap)
            return data[a:pos[0]]

        e = d.Engine(**kw)
        r = e.convert_stream_flac(read, out.append, total_bytes_per_channel=STREAM_BYTES, chunk_bytes_per_channel=STREAM_CHUNK, effort=1, **how)
        e.close()
        return out, r

    plain, stats = run()
    meter = d.LoudMeter(ch, rate)
    measured, r = run(loud=meter, md5=md5, verify=check)
    mstats = r[0] if (md5 or check) else r
    got = meter.finish()
    assert measured == plain and mstats.samples_per_channel == stats.samples_per_channel == want_pcm.size // 6 and mstats.blocks == stats.blocks == 12
    cells, io = d.loud_measure_host(ch, depth, rate, want_pcm)
    ref = d.LoudMeter(ch, rate)
    ref.add(cells, has_partial=True)
    want = ref.finish()
    assert io.subblocks == 5 and want.valid == 1 and want.blocks_total == 2
    assert bytes(got) == bytes(want), (got.lufs, want.lufs, got.peak, want.peak)
    if md5:
        import hashlib
        assert r[-1] == hashlib.md5(want_pcm.tobytes()).digest()
    with pytest.raises(d.D2DError) as ei:                                  # a meter for another channel count is refused
        run(loud=d.LoudMeter(1, rate))
    assert ei.value.code == ERR_PARAM and "channel count" in ei.value.message


@gpu
@pytest.mark.parametrize("effort", (0, 12))
@pytest.mark.parametrize("channels", (2, 1))
def test_cli_replaygain_writes_the_host_sinks_file(engine_lib, tmp_path, channels, effort):
    """--gpu-flac --flac-md5 --replaygain against the host sink's --replaygain: equal in every byte; `verify` accepts both; the tag holds
    what the host twin measures on the PCM of a plain conversion; without the switch no field is written"""
    d = engine_lib
    if not os.path.exists(CLI):
        d.build_library()
    n = 4096 * 44 + 500                                                   # 45181 frames at 88.2 kHz: 5 sub-blocks and a partial one, two 400 ms blocks
    chans = [synth("sine", n, seed=7), synth("pink", n, seed=8, amp=0.098)][:channels]
    for name in ("host", "gpu", "off"):
        (tmp_path / name).mkdir()
        write_dsf(str(tmp_path / name / "y.dsf"), chans)
    args = [CLI, "convert", "-o", "f", "-r", "88200", "-b", "24", "-d", "T", "-q", "--flac-effort", str(effort)]
    subprocess.check_call(args + ["--replaygain", str(tmp_path / "host" / "y.dsf")])
    subprocess.check_call(args + ["--gpu-flac", "--flac-md5", "--replaygain"] + (["--flac-verify"] if effort else []) + [str(tmp_path / "gpu" / "y.dsf")])
    subprocess.check_call(args + [str(tmp_path / "off" / "y.dsf")])
    h, g, o = ((tmp_path / k / "y.flac").read_bytes() for k in ("host", "gpu", "off"))
    assert g == h                                                          # equal in every byte
    assert b"REPLAYGAIN" not in o and o[:4] == b"fLaC" and len(h) > len(o)
    fields = vorbis_fields(str(tmp_path / "gpu" / "y.flac"))
    assert [f.split("=")[0] for f in fields] == ["REPLAYGAIN_REFERENCE_LOUDNESS", "REPLAYGAIN_TRACK_GAIN", "REPLAYGAIN_TRACK_PEAK"]
    assert fields[0] == "REPLAYGAIN_REFERENCE_LOUDNESS=-18.00 LUFS"
    assert fields[1] != "REPLAYGAIN_TRACK_GAIN=+00.00 dB"                  # (the placeholder, and what silence gets)
    assert re.fullmatch(r"REPLAYGAIN_TRACK_GAIN=[+-]\d\d\.\d\d dB", fields[1]) and re.fullmatch(r"REPLAYGAIN_TRACK_PEAK=\d\.\d{6}", fields[2])
    r = subprocess.run([CLI, "verify", str(tmp_path / "gpu" / "y.flac"), str(tmp_path / "host" / "y.flac")], capture_output=True, text=True)
    assert r.returncode == 0 and [l.endswith(": ok") for l in r.stdout.splitlines()] == [True, True], (r.stdout, r.stderr)
    if effort == 0:
        # `levels --loudness`: the same measurement on the float frames of the level check (no dither, no rounding to 24 bits: the tag's
        # two decimals and the line's two decimals may differ by a unit of the last place each, and by nothing more)
        lv = subprocess.run([CLI, "levels", "-r", "88200", "--loudness", str(tmp_path / "off" / "y.dsf")], capture_output=True, text=True)
        m = re.fullmatch(r"y\.dsf: (-?\d+\.\d{4}) dBFS, (-?\d+\.\d\d) LUFS\nHighest peak: -?\d+\.\d{4} dBFS\n", lv.stdout)
        assert lv.returncode == 0 and m, (lv.stdout, lv.stderr)
        gain = float(fields[1].split("=")[1].split()[0])
        assert abs((-18.0 - float(m.group(2))) - gain) <= 0.02, (m.group(2), gain)
        plain = subprocess.run([CLI, "levels", "-r", "88200", str(tmp_path / "off" / "y.dsf")], capture_output=True, text=True)
        assert plain.stdout == f"y.dsf: {m.group(1)} dBFS\nHighest peak: {m.group(1)} dBFS\n"
