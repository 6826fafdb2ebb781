"""True peak on the GPU (include/dsd2dxd_amd.h, "Loudness where the PCM is": d2d_true_peak_measure_device, the stream driver
d2d_convert_stream_flac_loud with a meter whose true peak is switched on, the CLI's --replaygain --true-peak and `levels --true-peak`).
The reference of every double is the host twin, d2d_true_peak_measure_host, which compiles the same true_peak.h and which
tests/test_true_peak_cpu.py holds to an independent restatement in integers: device doubles must be the twin's BYTES, no tolerance.  Rate
8000 makes a sub-block 800 frames; every call measures a few thousand frames per file.  A tile of the kernel is 256 / channels * 8
frames: 2048 for mono, 256 for eight channels, so 800 frames are several tiles for three channels and more, and the 88.2 kHz case is
several tiles for stereo."""
import os
import re
import subprocess

import numpy as np
import pytest

import true_peak_ref as T
from helpers import pack_layout, synth, write_dsf
from test_gpu_containment import Arena, describe, fill_bytes, violations
from test_gpu_flac_md5 import _dev, _engine_kw, _host, plain_pcm, upload
from test_loudness_cpu import vorbis_fields
from test_true_peak_cpu import MAGNITUDES, noise_pcm, worst_case_pcm

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "dsd2dxd_amd", "dsd2dxd_amd_cli")
ERR_PARAM, ERR_CAPACITY = -1, -20
MAXF = 64           # the files of one launch: MAXF in dsd2dxd_amd/csrc/loud/d2d_true_peak.hip
SLACK = 3           # doubles of capacity behind what a call writes: they must stay as they were
EE = np.frombuffer(bytes([0xEE] * 8), dtype=np.float64)[0]


def twin(d, ch, depth, rate, piece, first_frame, first_subblock, final):
    """the host twin's doubles of one file as bytes, and its counts (frames == 0: none, the counts a caller's record keeps)"""
    if piece.size == 0:
        return b"", (None, 0, None)
    peaks, io = d.true_peak_measure_host(ch, depth, rate, piece, first_frame=first_frame, first_subblock=first_subblock, final=final)
    return peaks.tobytes(), (io.subblocks, io.peaks_out, io.next_subblock)


def device_call(d, ch, depth, rate, pieces, firsts=None, subs=None, final=True, stream=None):
    """one d2d_true_peak_measure_device call with one piece per file; returns per file (bytes written, counts) after checking that the
    capacity behind peaks_out was left alone"""
    n = len(pieces)
    firsts, subs = firsts or [0] * n, subs or [0] * n
    want = [twin(d, ch, depth, rate, p, firsts[i], subs[i], final) for i, p in enumerate(pieces)]
    caps = [w[1][1] + SLACK for w in want]
    starts = np.concatenate([[0], np.cumsum(caps)]).astype(int)
    t_peaks = _dev(np.full(int(starts[-1]), EE, dtype=np.float64))
    t_pcm, ptrs = upload(pieces)
    ios = (d.TruePeakIO * n)()
    fb = ch * T.sample_bytes(depth)
    for i in range(n):
        ios[i] = d.TruePeakIO(ptrs[i], pieces[i].size // fb, firsts[i], subs[i], int(final), 0, t_peaks.data_ptr() + 8 * int(starts[i]), caps[i], 111, 222, 333)
    d.true_peak_measure_device(ch, depth, rate, ios, stream)
    got = _host(t_peaks)
    out = []
    for i in range(n):
        if pieces[i].size == 0:                                            # left alone, the counts too
            assert (ios[i].subblocks, ios[i].peaks_out, ios[i].next_subblock) == (111, 222, 333)
            k = 0
        else:
            assert (ios[i].subblocks, ios[i].peaks_out, ios[i].next_subblock) == want[i][1], (i, want[i][1])
            k = ios[i].peaks_out
        region = got[starts[i]:starts[i + 1]]
        assert region[k:].tobytes() == bytes([0xEE]) * (8 * (caps[i] - k)), f"file {i}: doubles behind peaks_out were written"
        out.append(region[:k].tobytes())
    return out, want


@gpu
@pytest.mark.parametrize("depth", (16, 20, 24, 32))
@pytest.mark.parametrize("channels", (1, 2, 3, 6, 8))
def test_device_doubles_are_the_host_twins_bytes(engine_lib, channels, depth):
    """four files in one call -- 0 frames, under one sub-block, exactly 3 sub-blocks, 4 sub-blocks and a partial -- final and not"""
    rate, S = 8000, 800
    pieces = [noise_pcm(n, channels, depth, seed=10 * channels + k) if n else np.zeros(0, dtype=np.uint8)
              for k, n in enumerate((0, 300, 3 * S, 4 * S + 123))]
    for final in (True, False):
        got, want = device_call(engine_lib, channels, depth, rate, pieces, final=final)
        rows = [len(g) // (8 * channels) for g in got]
        assert rows == ([0, 1, 3, 5] if final else [0, 0, 3, 4])
        for i in range(4):
            assert got[i] == want[i][0], f"file {i}, final {final}: the device doubles are not the host twin's bytes"


@gpu
def test_stereo_24_bit_at_88200_over_several_tiles(engine_lib):
    """a sub-block of 8820 frames is nine tiles of 1024 for stereo, the last of 628; three sub-blocks and a partial row of 1000"""
    rate, S = 88200, 8820
    piece = noise_pcm(3 * S + 1000, 2, 24, seed=88)
    got, want = device_call(engine_lib, 2, 24, rate, [piece])
    assert len(got[0]) == 4 * 2 * 8 and got[0] == want[0][0]
    assert got[0] == T.cells(piece, 2, 24, rate).tobytes()                 # ... and the twin is the reference's, here too


@gpu
def test_more_files_than_one_launch_holds(engine_lib):
    """MAXF + 1 mono 16-bit files of different lengths, some empty, in one call: the library cuts it into two launches"""
    S = 800
    pieces = [noise_pcm(S + 37 * k, 1, 16, seed=k) if k % 9 else np.zeros(0, dtype=np.uint8) for k in range(MAXF + 10)]
    assert sum(1 for p in pieces if p.size) == MAXF + 1
    got, want = device_call(engine_lib, 1, 16, 8000, pieces)
    assert [i for i in range(len(pieces)) if got[i] != want[i][0]] == []
    assert sum(len(g) for g in got) // 8 >= 2 * (MAXF + 1)


@gpu
@pytest.mark.parametrize("depth", (16, 24))
def test_worst_case_sums(engine_lib, depth):
    """the rail-level streams of tests/test_true_peak_cpu.py, one file per (phase, place) in one call: the extreme output is the first
    frame of a sub-block, the last frame of one, the last frame of a partial row, frame 11 of the stream"""
    rate, S = 8000, 800
    frames = 2 * S + 300
    cases = [(phase, at, row) for phase in range(4) for at, row in ((S, 1), (2 * S - 1, 1), (frames - 1, 2), (11, 0))]
    made = [worst_case_pcm(phase, at, frames, depth, channels=2, channel=1) for phase, at, row in cases]
    got, want = device_call(engine_lib, 2, depth, rate, [m[0] for m in made])
    for i, (phase, at, row) in enumerate(cases):
        assert got[i] == want[i][0], (phase, at)
        cells = np.frombuffer(got[i], dtype=np.float64).reshape(3, 2)
        assert cells[row, 1] >= made[i][1] and np.all(cells[:, 0] == 0.0)
        if phase in (1, 2):
            rail = ((1 << (depth - 1)) - 1) / (1 << (depth - 1))
            assert cells[row, 1] == made[i][1] == MAGNITUDES[phase] / 8192.0 * rail == cells.max(), (phase, at)


@gpu
@pytest.mark.parametrize("channels,depth", [(2, 24), (3, 16), (1, 32)])
def test_a_stream_cut_into_calls_with_the_minimum_history(engine_lib, channels, depth):
    """one call per sub-block, each with PCM from frame max(0, j S - 11) and nothing more in front; then ragged cuts; the doubles are
    those of the whole stream in one call.  (A piece that begins eleven frames before a sub-block is not 16-byte aligned in the stream:
    every piece is uploaded to an aligned place of its own.)"""
    d, rate, S = engine_lib, 8000, 800
    frames = 4 * S + 55
    pcm = noise_pcm(frames, channels, depth, seed=21)
    fb = channels * T.sample_bytes(depth)
    whole, _ = twin(d, channels, depth, rate, pcm, 0, 0, True)
    for ends in ([S * k for k in range(1, 5)] + [frames], [S // 2, S + 3, 3 * S - 1, 3 * S, frames]):
        got, nxt = b"", 0
        for end in ends:
            first = max(0, nxt * S - 11)
            (peaks,), want = device_call(d, channels, depth, rate, [pcm[first * fb:end * fb]], [first], [nxt], final=end == frames)
            assert peaks == want[0][0]
            got += peaks
            nxt = end // S
        assert got == whole, ends


@gpu
def test_a_nine_byte_stride_and_a_length_that_is_no_multiple_of_16(engine_lib):
    """three channels of 24 bits: frames of nine bytes, so frames and tile edges straddle the 16-byte words of the stage, and files whose
    last 16-byte word is partial in every way (lengths 9 n mod 16 = 9, 2, 11, 4, 13, 6, 15, 8, 1, ...)"""
    rate, S = 8000, 800
    lengths = [S + k for k in range(1, 17)]
    assert sorted({(9 * n) % 16 for n in lengths}) == list(range(16))
    pieces = [noise_pcm(n, 3, 24, seed=n) for n in lengths]
    got, want = device_call(engine_lib, 3, 24, rate, pieces)
    assert [lengths[i] for i in range(len(pieces)) if got[i] != want[i][0]] == []


@gpu
@pytest.mark.parametrize("complement", (False, True))
def test_a_call_writes_its_doubles_and_reads_its_frames(engine_lib, complement):
    """pcm and peaks each in an arena between 32 KiB guards, files back to back, capacities exact, two complementary fills: exactly
    peaks_out doubles per file are written and they are the twin's whatever lies behind the declared frames; refused calls change no byte"""
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
        x = (d.TruePeakIO * n)()
        for i in range(n):
            x[i] = d.TruePeakIO(t_in.data_ptr() + a_in.starts[i], frames[i], firsts[i], subs[i], 1, 0, t_out.data_ptr() + a_out.starts[i], len(want[i][0]) // 8, 111, 222, 333)
        for (i, field), v in (change or {}).items():
            setattr(x[i], field, getattr(x[i], field) + v)
        return x

    def check(what, peaks):
        v = violations(a_out, _host(t_out), f_out, peaks)
        assert not v, what + ": " + describe(v)
        assert np.array_equal(_host(t_in), f_in), what + ": the pcm arena changed"

    refusals = [((ch, 17, rate), {}, ERR_PARAM, "bit depth"), ((9, depth, rate), {}, ERR_PARAM, "channel"), ((ch, depth, 8004), {}, ERR_PARAM, "rate"),
                ((ch, depth, rate), {(3, "pcm"): 8}, ERR_PARAM, "aligned"), ((ch, depth, rate), {(0, "peaks"): 4}, ERR_PARAM, "aligned"),
                ((ch, depth, rate), {(4, "first_frame"): 2 * S - 10}, ERR_PARAM, "history"), ((ch, depth, rate), {(0, "first_frame"): 1}, ERR_PARAM, "history"),
                ((ch, depth, rate), {(4, "peaks_capacity"): -1}, ERR_CAPACITY, "peaks_capacity")]
    for args, kw, code, text in refusals:
        x = ios(kw)
        with pytest.raises(d.D2DError) as ei:
            d.true_peak_measure_device(*args, x)
        assert ei.value.code == code and text in ei.value.message, (args, kw, ei.value)
        assert all((x[i].subblocks, x[i].peaks_out, x[i].next_subblock) == (111, 222, 333) for i in range(n)), "a refused call wrote counts"
        check("refused: " + text, [None] * n)
    x = ios()
    d.true_peak_measure_device(ch, depth, rate, x)
    assert [x[i].peaks_out for i in range(n)] == [9, 222, 3, 9, 6]
    check("measured", [np.frombuffer(w[0], dtype=np.uint8) if w[0] else None for w in want])
    d.true_peak_measure_device(ch, depth, rate, (d.TruePeakIO * 0)())     # n_files == 0: nothing
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
    peaks = _dev(np.full(16, EE, dtype=np.float64))
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    io = (d.FileIO * 1)()
    io[0].dsd, io[0].bytes_per_channel, io[0].pcm, io[0].pcm_capacity_bytes = dsd.data_ptr(), nbytes, pcm.data_ptr(), pcm.numel()
    e.translate_batch_device(io, s.cuda_stream)
    nf = io[0].frames_out
    pio = (d.TruePeakIO * 1)()
    pio[0] = d.TruePeakIO(pcm.data_ptr(), nf, 0, 0, 1, 0, peaks.data_ptr(), 16, 0, 0, 0)
    d.true_peak_measure_device(ch, depth, rate, pio, s.cuda_stream)
    s.synchronize()
    e.close()
    frames = _host(pcm)[:nf * fb]
    want, counts = twin(d, ch, depth, rate, frames, 0, 0, True)
    assert nf // 8820 == 3 and nf % 8820 and (pio[0].subblocks, pio[0].peaks_out, pio[0].next_subblock) == counts == (3, 8, 3)
    assert _host(peaks).tobytes()[:len(want)] == want and frames.any()


STREAM_BYTES = 4096 * 48            # per channel: 49152 frames at 88.2 kHz, 5 sub-blocks and a partial one, 12 FLAC blocks
STREAM_CHUNK = 5 * 4096             # ten chunks, the last three fifths of one


@gpu
@pytest.mark.parametrize("md5,check", [(False, False), (True, True)], ids=("plain", "hashed-verified"))
def test_stream_driver_feeds_the_meters_true_peak(engine_lib, md5, check):
    """d2d_convert_stream_flac_loud with a meter whose true peak is on: the frames and stats of the call without the meter, the result of
    the meter without the switch, and the true peak the host twin gives over the whole PCM of the plain conversion.  With the switch
    off the driver writes the same bytes and the meter has no true peak: no true-peak call was made for it."""
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
    off = d.LoudMeter(ch, rate)
    measured_off, _ = run(loud=off, md5=md5, verify=check)
    meter = d.LoudMeter(ch, rate, true_peak=True)
    measured, r = run(loud=meter, md5=md5, verify=check)
    mstats = r[0] if (md5 or check) else r
    assert measured == plain == measured_off and mstats.samples_per_channel == stats.samples_per_channel == want_pcm.size // 6 and mstats.blocks == 12
    assert bytes(meter.finish()) == bytes(off.finish())
    with pytest.raises(d.D2DError) as ei:                                  # the switch off: no rows came
        off.true_peak()
    assert ei.value.code == ERR_PARAM
    peaks, io = d.true_peak_measure_host(ch, depth, rate, want_pcm)
    assert io.subblocks == 5 and io.peaks_out == 12
    want = max(peaks.max(), meter.finish().peak)
    assert meter.true_peak() == want and want >= T.sample_peak(want_pcm, ch, depth)
    assert peaks.tobytes() == T.cells(want_pcm, ch, depth, rate).tobytes()
    if md5:
        import hashlib
        assert r[-1] == hashlib.md5(want_pcm.tobytes()).digest()


@gpu
@pytest.mark.parametrize("effort", (0, 12))
@pytest.mark.parametrize("channels", (2, 1))
def test_cli_true_peak_writes_the_host_sinks_file(engine_lib, tmp_path, channels, effort):
    """--gpu-flac --flac-md5 --replaygain --true-peak against the host sink's --replaygain --true-peak: equal in every byte; `verify`
    accepts both; against --replaygain alone nothing but the eight characters of REPLAYGAIN_TRACK_PEAK moves, and they hold what the
    host twin measures on the file's own decoded samples; `levels --true-peak` has the line format"""
    d = engine_lib
    if not os.path.exists(CLI):
        d.build_library()
    n = 4096 * 44 + 500                                                   # 45181 frames at 88.2 kHz: 5 sub-blocks and a partial one
    chans = [synth("sine", n, seed=7), synth("pink", n, seed=8, amp=0.098)][:channels]
    for name in ("host", "gpu", "sample"):
        (tmp_path / name).mkdir()
        write_dsf(str(tmp_path / name / "y.dsf"), chans)
    args = [CLI, "convert", "-r", "88200", "-b", "24", "-d", "T", "-q", "--flac-effort", str(effort)]
    subprocess.check_call(args + ["-o", "f", "--replaygain", "--true-peak", str(tmp_path / "host" / "y.dsf")])
    subprocess.check_call(args + ["-o", "f", "--gpu-flac", "--flac-md5", "--replaygain", "--true-peak"] + (["--flac-verify"] if effort else []) + [str(tmp_path / "gpu" / "y.dsf")])
    subprocess.check_call(args + ["-o", "f", "--replaygain", str(tmp_path / "sample" / "y.dsf")])
    h, g, s = ((tmp_path / k / "y.flac").read_bytes() for k in ("host", "gpu", "sample"))
    assert g == h                                                          # equal in every byte
    pos, last = 4, False                                                   # the frames lie behind the metadata blocks
    while not last:
        last, pos = bool(g[pos] & 0x80), pos + 4 + int.from_bytes(g[pos + 1:pos + 4], "big")
    decoded, nf, chk = d.flac_decode_host(channels, 24, g[pos:], capacity=(45181 + 4096) * channels * 3)
    pcm = np.frombuffer(decoded, dtype=np.uint8)
    assert nf == 45181 and chk.bad_blocks == 0
    peaks, io = d.true_peak_measure_host(channels, 24, 88200, pcm)
    sample = T.sample_peak(pcm, channels, 24)
    want = max(peaks.max(), sample)
    diff = [i for i in range(len(h)) if h[i] != s[i]]
    assert len(h) == len(s) and bool(diff) == ("%.6f" % want != "%.6f" % sample) and (not diff or max(diff) - min(diff) < 8)
    print(f"{channels} ch effort {effort}: true peak {want:.6f}, sample peak {sample:.6f}")
    fields = vorbis_fields(str(tmp_path / "gpu" / "y.flac"))
    assert fields[2] == "REPLAYGAIN_TRACK_PEAK=%.6f" % want and fields[:2] == vorbis_fields(str(tmp_path / "sample" / "y.flac"))[:2]
    r = subprocess.run([CLI, "verify", str(tmp_path / "gpu" / "y.flac"), str(tmp_path / "host" / "y.flac")], capture_output=True, text=True)
    assert r.returncode == 0 and [l.endswith(": ok") for l in r.stdout.splitlines()] == [True, True], (r.stdout, r.stderr)
    if effort == 0:
        # `levels --true-peak`: the same measurement on the float frames of the level check (no dither, no rounding to 24 bits)
        lv = subprocess.run([CLI, "levels", "-r", "88200", "--true-peak", str(tmp_path / "sample" / "y.dsf")], capture_output=True, text=True)
        m = re.fullmatch(r"y\.dsf: (-?\d+\.\d{4}) dBFS, (-?\d+\.\d{4}) dBTP\nHighest peak: (-?\d+\.\d{4}) dBFS\n", lv.stdout)
        assert lv.returncode == 0 and m and m.group(1) == m.group(3), (lv.stdout, lv.stderr)
        assert float(m.group(2)) >= float(m.group(1)) - 0.0002 and abs(float(m.group(2)) - 20 * np.log10(want)) <= 0.01, (m.groups(), want)
        both = subprocess.run([CLI, "levels", "-r", "88200", "--loudness", "--true-peak", str(tmp_path / "sample" / "y.dsf")], capture_output=True, text=True)
        assert re.fullmatch(r"y\.dsf: %s dBFS, -?\d+\.\d\d LUFS, %s dBTP\nHighest peak: %s dBFS\n" % tuple(re.escape(m.group(k)) for k in (1, 2, 1)), both.stdout), both.stdout
        plain = subprocess.run([CLI, "levels", "-r", "88200", str(tmp_path / "sample" / "y.dsf")], capture_output=True, text=True)
        assert plain.stdout == f"y.dsf: {m.group(1)} dBFS\nHighest peak: {m.group(1)} dBFS\n"
