"""Loudness, the host side (include/dsd2dxd_amd.h, "Loudness where the PCM is"): d2d_loud_coefficients, d2d_loud_measure_host -- the CPU
twin of the GPU call, built on dsd2dxd_amd/csrc/loud/loud_meter.h, the source the kernel compiles too -- and the integration
(d2d_loud_create / _add / _finish) against tests/loudness_ref.py, an independent numpy / scipy restatement; the FLAC sink's --replaygain
fields through tools/loud_sink_probe.cpp; the refusals; a sanitised run of tools/loud_fuzz.cpp.  No GPU.  tests/test_gpu_loudness.py
holds the device call to this twin byte for byte.

Bounds.  Energies: 1e-10 relative, against the reference with the same restarts and against one uninterrupted lfilter pass -- three
orders over the 1.1e-13 that the restart itself costs, seven under the 2.3e-3 that moves a tag's last digit.  Peaks: exact.  Integrated
loudness of the sines: the figures of the standard's formulas +- 0.005 LU.  The gated sequence: 1e-6 LU against the reference."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import loudness_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "dsd2dxd_amd", "dsd2dxd_amd_cli")
CSRC = os.path.join(ROOT, "dsd2dxd_amd", "csrc")
ERR_PARAM, ERR_CAPACITY = -1, -20
DEPTHS = (16, 20, 24, 32)
CHANNELS = (1, 2, 6, 8)
RATES = (8000, 88200)
ENERGY_RTOL = 1e-10


def noise_pcm(frames, channels, depth, seed, dc=0.3, amp=0.25):
    """packed frames of seeded noise around a DC offset (the offset is what a restarted high-pass has to forget)"""
    rng = np.random.default_rng(seed)
    x = dc + amp * rng.standard_normal((frames, channels))
    x[:, channels - 1] *= 0.5                                           # the channels differ
    if depth == 32:
        return R.pack(x.astype(np.float32), 32)
    bits = 20 if depth == 20 else depth
    full = 1 << (bits - 1)
    return R.pack(np.clip(np.round(x * full), -full, full - 1).astype(np.int64), depth)


def measure(d, channels, depth, rate, pcm, **kw):
    cells, io = d.loud_measure_host(channels, depth, rate, pcm, **kw)
    return cells, io


def integrated(d, channels, rate, cells, io, weights=None):
    m = d.LoudMeter(channels, rate, weights)
    m.add(cells, has_partial=io.cells_out > io.subblocks * channels)
    r = m.finish()
    m.close()
    return r


# ---- coefficients ----

def test_coefficients_at_48000_are_the_standards_table(engine_lib):
    k = engine_lib.loud_coefficients(48000)
    table = [1.53512485958697, -2.69169618940638, 1.19839281085285, -1.69065929318241, 0.73248077421585,
             1.0, -2.0, 1.0, -1.99004745483398, 0.99007225036621]
    assert np.max(np.abs(np.array(k) - np.array(table))) <= 1e-12, k


@pytest.mark.parametrize("rate", (8000, 11020, 44100, 88200, 96000, 352800, 1411200))
def test_coefficients_match_the_closed_form(engine_lib, rate):
    k, want = np.array(engine_lib.loud_coefficients(rate)), R.ten(rate)
    assert np.all(np.abs(k - want) <= 1e-12 * np.abs(want)), (k, want)


def test_structures_have_the_public_layout(engine_lib):
    d = engine_lib
    assert C.sizeof(d.LoudCell) == 16 and C.sizeof(d.LoudIO) == 80 and C.sizeof(d.LoudResult) == 48
    assert (d.LoudIO.cells.offset, d.LoudIO.subblocks.offset, d.LoudIO.next_subblock.offset) == (40, 56, 72)


# ---- cells ----

@pytest.mark.parametrize("rate", RATES)
@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("channels", CHANNELS)
def test_cells_of_the_host_twin_against_the_reference(engine_lib, channels, depth, rate):
    """5 sub-blocks and a partial sixth: against the reference with the same restarts, and against one uninterrupted pass"""
    S = rate // 10
    frames = 5 * S + S // 3
    pcm = noise_pcm(frames, channels, depth, seed=channels * 100 + depth)
    cells, io = measure(engine_lib, channels, depth, rate, pcm)
    assert (io.subblocks, io.cells_out, io.next_subblock) == (5, 6 * channels, 5) and cells.shape == (6, channels, 2)
    x = R.to_float(pcm, channels, depth)
    for restart in (True, False):
        want = R.cells(x, rate, restart=restart)
        err = np.max(np.abs(cells[:, :, 0] - want[:, :, 0]) / want[:, :, 0])
        print(f"ch {channels} depth {depth} rate {rate} restart {restart}: energy error {err:.3g} relative")
        assert err <= ENERGY_RTOL, (restart, err)
        assert np.array_equal(cells[:, :, 1], want[:, :, 1]), "peaks must be exact"
    # a call that is not final leaves the partial sub-block alone
    cells_nf, io_nf = measure(engine_lib, channels, depth, rate, pcm, final=False)
    assert (io_nf.subblocks, io_nf.cells_out, io_nf.next_subblock) == (5, 5 * channels, 5)
    assert cells_nf.tobytes() == cells[:5].tobytes()


@pytest.mark.parametrize("channels,depth,rate", [(2, 24, 8000), (3, 16, 8010), (1, 32, 8000), (6, 20, 11020)])
def test_cutting_at_every_subblock_boundary_gives_the_same_bytes(engine_lib, channels, depth, rate):
    """one call per sub-block, each holding the minimum pre-roll and nothing more; then two sub-blocks per call, then ragged cuts"""
    S = rate // 10
    frames = 7 * S + 17
    pcm = noise_pcm(frames, channels, depth, seed=7)
    fb = channels * R.sample_bytes(depth)
    whole, io = measure(engine_lib, channels, depth, rate, pcm)
    assert io.cells_out == 8 * channels
    for ends in ([S * k for k in range(1, 8)] + [frames], [2 * S, 4 * S, 6 * S, frames], [5, S - 1, S + 1, 3 * S + 9, 3 * S + 9, 6 * S, frames - 1, frames]):
        got, nxt = [], 0
        for end in ends:
            first = max(0, nxt - 2) * S
            piece = pcm[first * fb:end * fb]
            if piece.size == 0:
                continue
            cells, cio = measure(engine_lib, channels, depth, rate, piece, first_frame=first, first_subblock=nxt, final=end == frames)
            assert cio.next_subblock == end // S and cio.subblocks == end // S - nxt
            got.append(cells)
            nxt = cio.next_subblock
        assert np.concatenate(got).tobytes() == whole.tobytes(), ends


# ---- integration ----

def sine_pcm(rate, channels, seconds=3, f=997.0):
    n = rate * seconds
    x = np.round(np.sin(2 * np.pi * f * np.arange(n) / rate) * (2 ** 23 - 1)).astype(np.int64)
    return R.pack(np.repeat(x[:, None], channels, axis=1), 24)


@pytest.mark.parametrize("rate,channels,want", [(48000, 1, -3.010), (48000, 2, -3.010 + 3.010), (88200, 1, -3.026), (8000, 1, -2.996)])
def test_full_scale_sine(engine_lib, rate, channels, want):
    pcm = sine_pcm(rate, channels)
    cells, io = measure(engine_lib, channels, 24, rate, pcm)
    r = integrated(engine_lib, channels, rate, cells, io)
    print(f"997 Hz full scale, {channels} ch at {rate}: {r.lufs:.6f} LUFS")
    assert r.valid == 1 and abs(r.lufs - want) <= 0.005, r.lufs
    assert r.gain_db == -18.0 - r.lufs and r.peak == (2 ** 23 - 1) / 2 ** 23
    assert r.blocks_total == 27 and r.blocks_gated == 0


def test_loud_quiet_silent_sequence_passes_both_gates(engine_lib):
    """2 s loud, 2 s 30 dB quieter (above -70 LUFS, under the relative gate), 2 s of digital silence (under the absolute gate)"""
    rate, ch = 8000, 2
    rng = np.random.default_rng(11)
    loud = 0.2 * rng.standard_normal((2 * rate, ch))
    x = np.concatenate([loud, loud * 10 ** (-30 / 20), np.zeros((2 * rate, ch))])
    pcm = R.pack(np.round(x * 2 ** 23).clip(-2 ** 23, 2 ** 23 - 1).astype(np.int64), 24)
    cells, io = measure(engine_lib, ch, 24, rate, pcm)
    r = integrated(engine_lib, ch, rate, cells, io)
    ref = R.integrate(R.cells(R.to_float(pcm, ch, 24), rate), rate, io.subblocks)
    assert ref["removed_absolute"] > 0 and ref["removed_relative"] > 0, ref
    print(f"sequence: {r.lufs:.9f} LUFS, reference {ref['lufs']:.9f}; gates removed {ref['removed_absolute']} + {ref['removed_relative']} of {ref['blocks_total']}")
    assert r.valid == 1 and abs(r.lufs - ref["lufs"]) <= 1e-6
    assert r.blocks_total == ref["blocks_total"] == 57
    assert r.blocks_gated == ref["removed_absolute"] + ref["removed_relative"]
    assert abs(r.gain_db - ref["gain_db"]) <= 1e-6 and r.peak == ref["peak"]


def test_silence_is_invalid_and_its_gain_is_zero(engine_lib):
    for frames in (0, 100, 8000 * 2):
        pcm = np.zeros(frames * 2 * 2, dtype=np.uint8)
        cells, io = measure(engine_lib, 2, 16, 8000, pcm)
        r = integrated(engine_lib, 2, 8000, cells, io)
        assert (r.valid, r.lufs, r.gain_db, r.peak) == (0, 0.0, 0.0, 0.0)
        assert r.blocks_total == r.blocks_gated == max(0, frames // 800 - 3)


def test_six_channels_ignore_the_lfe_and_weight_the_surrounds(engine_lib):
    rate, ch = 8000, 6
    pcm = noise_pcm(2 * rate, ch, 24, seed=3, dc=0.0, amp=0.1)
    x = R.to_float(pcm, ch, 24)
    cells, io = measure(engine_lib, ch, 24, rate, pcm)
    r = integrated(engine_lib, ch, rate, cells, io)
    ref = R.integrate(R.cells(x, rate), rate, io.subblocks, weights=[1, 1, 1, 0, 1.41, 1.41])
    assert abs(r.lufs - ref["lufs"]) <= 1e-6
    # the LFE alone moves nothing but the peak; a surround alone is 10 log10(1.41) over a front channel alone
    only = lambda c: R.pack(np.where(np.arange(ch) == c, 1, 0) * np.round(x * 2 ** 23).astype(np.int64), 24)
    res = {}
    for c in (0, 3, 4):
        cc, cio = measure(engine_lib, ch, 24, rate, only(c))
        res[c] = integrated(engine_lib, ch, rate, cc, cio)
    assert res[3].valid == 0 and res[3].peak > 0
    # (the channels carry different noise: compare each with the reference on its own weights instead of with each other)
    for c, w in ((0, 1.0), (4, 1.41)):
        ref_c = R.integrate(R.cells(R.to_float(only(c), ch, 24), rate), rate, io.subblocks, weights=[w if k == c else 0 for k in range(ch)])
        assert abs(res[c].lufs - ref_c["lufs"]) <= 1e-6
    # a caller's own weights
    own = integrated(engine_lib, ch, rate, cells, io, weights=[1.0] * 6)
    assert abs(own.lufs - R.integrate(R.cells(x, rate), rate, io.subblocks, weights=[1.0] * 6)["lufs"]) <= 1e-6 and own.lufs > r.lufs - 10


def test_a_partial_subblock_contributes_its_peak_only(engine_lib):
    rate, S = 8000, 800
    x = np.zeros((4 * S + 10, 1), dtype=np.int64)
    x[:4 * S, 0] = np.round(0.1 * 2 ** 15 * np.sin(2 * np.pi * 440 * np.arange(4 * S) / rate))
    x[4 * S + 3, 0] = 30000                                              # the peak lies in the partial sub-block
    pcm = R.pack(x, 16)
    cells, io = measure(engine_lib, 1, 16, rate, pcm)
    assert io.subblocks == 4 and io.cells_out == 5
    r = integrated(engine_lib, 1, rate, cells, io)
    without, io4 = measure(engine_lib, 1, 16, rate, pcm[:4 * S * 2])
    r4 = integrated(engine_lib, 1, rate, without, io4)
    assert r.peak == 30000 / 32768 and r4.peak < 0.11 and r.lufs == r4.lufs and r.blocks_total == 1
    m = engine_lib.LoudMeter(1, rate)
    m.add(cells, has_partial=True)
    with pytest.raises(engine_lib.D2DError) as ei:                       # nothing comes behind the partial sub-block
        m.add(cells[:1])
    assert ei.value.code == -40


# ---- refusals ----

def test_refusals_return_their_codes_and_write_nothing(engine_lib):
    d = engine_lib
    L = d.lib()
    S = 800
    pcm = noise_pcm(4 * S, 2, 16, seed=1)
    cells = np.full((16, 2), 7.5, dtype=np.float64)

    def io(**kw):
        v = dict(pcm=pcm.ctypes.data, frames=4 * S, first_frame=0, first_subblock=0, final=1, cells=cells.ctypes.data, cells_capacity=16)
        v.update(kw)
        return d.LoudIO(v["pcm"], v["frames"], v["first_frame"], v["first_subblock"], v["final"], 0, v["cells"], v["cells_capacity"], 111, 222, 333)

    cases = [((2, 17, 8000), {}, ERR_PARAM, "bit depth"), ((2, 12, 8000), {}, ERR_PARAM, "bit depth"),
             ((0, 16, 8000), {}, ERR_PARAM, "channel"), ((9, 16, 8000), {}, ERR_PARAM, "channel"),
             ((2, 16, 8005), {}, ERR_PARAM, "rate"), ((2, 16, 7990), {}, ERR_PARAM, "rate"), ((2, 16, 1411210), {}, ERR_PARAM, "rate"),
             ((2, 16, 8000), dict(pcm=None), ERR_PARAM, "non-null"), ((2, 16, 8000), dict(cells=None), ERR_PARAM, "non-null"),
             ((2, 16, 8000), dict(first_subblock=1, first_frame=1), ERR_PARAM, "pre-roll"),
             ((2, 16, 8000), dict(first_subblock=3, first_frame=S + 1, frames=3 * S - 1), ERR_PARAM, "pre-roll"),
             ((2, 16, 8000), dict(cells_capacity=7), ERR_CAPACITY, "cells_capacity")]
    for (ch, depth, rate), kw, code, text in cases:
        rec = io(**kw)
        rc = L.d2d_loud_measure_host(ch, depth, rate, C.byref(rec))
        assert rc == code and text in L.d2d_flac_error().decode(), ((ch, depth, rate), kw, rc, L.d2d_flac_error())
        assert (rec.subblocks, rec.cells_out, rec.next_subblock) == (111, 222, 333) and np.all(cells == 7.5)
    assert L.d2d_loud_measure_host(2, 16, 8000, None) == ERR_PARAM
    # the same call with the capacity it needs passes and writes exactly its 8 cells; frames == 0 leaves the record alone
    rec = io(cells_capacity=8)
    assert L.d2d_loud_measure_host(2, 16, 8000, C.byref(rec)) == 0 and rec.cells_out == 8 and np.all(cells[8:] == 7.5) and np.all(cells[:8] != 7.5)
    rec = io(frames=0, pcm=None, cells=None)
    assert L.d2d_loud_measure_host(2, 16, 8000, C.byref(rec)) == 0 and (rec.subblocks, rec.cells_out, rec.next_subblock) == (111, 222, 333)
    out = (C.c_double * 10)(*([5.0] * 10))
    assert L.d2d_loud_coefficients(8001, out) == ERR_PARAM and list(out) == [5.0] * 10
    assert L.d2d_loud_coefficients(8000, None) == ERR_PARAM
    h = C.c_void_p()
    assert L.d2d_loud_create(0, 8000, None, C.byref(h)) == ERR_PARAM and L.d2d_loud_create(9, 8000, None, C.byref(h)) == ERR_PARAM
    assert L.d2d_loud_create(2, 44101, None, C.byref(h)) == ERR_PARAM and L.d2d_loud_create(2, 8000, None, None) == ERR_PARAM and not h.value
    assert L.d2d_loud_add(None, cells.ctypes.data, 1, 0) == ERR_PARAM and L.d2d_loud_finish(None, None) == ERR_PARAM
    stream = L.d2d_convert_stream_flac_loud
    assert stream(*[t() for t in stream.argtypes]) == ERR_PARAM and "null meter" in L.d2d_flac_error().decode()      # (every argument null)


# ---- files ----

def vorbis_fields(path):
    """the fields of a FLAC file's VORBIS_COMMENT block, in order, and the block's position; None when there is no such block"""
    data = open(path, "rb").read()
    assert data[:4] == b"fLaC"
    pos, last = 4, False
    while not last:
        last, kind = bool(data[pos] & 0x80), data[pos] & 0x7F
        size = int.from_bytes(data[pos + 1:pos + 4], "big")
        if kind == 4:
            b = data[pos + 4:pos + 4 + size]
            n = struct.unpack_from("<I", b, 0)[0]
            at = 4 + n
            count = struct.unpack_from("<I", b, at)[0]
            at += 4
            fields = []
            for _ in range(count):
                n = struct.unpack_from("<I", b, at)[0]
                fields.append(b[at + 4:at + 4 + n].decode())
                at += 4 + n
            assert at == size
            return fields
        pos += 4 + size
    return None


@pytest.fixture(scope="module")
def sink_probe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("loud") / "loud_sink_probe")
    src = [os.path.join(ROOT, "tools", "loud_sink_probe.cpp"), os.path.join(CSRC, "host", "pcm_sink.cpp"), os.path.join(CSRC, "host", "id3_tag.cpp"),
           os.path.join(CSRC, "loud", "d2d_loud_host.cpp"), os.path.join(CSRC, "flac", "d2d_flac_host.cpp")]
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-o", exe] + src + ["-lpthread"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def id3_with_title(title):
    body = b"\x00" + title.encode("latin-1")
    frame = b"TIT2" + struct.pack(">I", len(body)) + b"\x00\x00" + body
    n = len(frame)
    return b"ID3\x03\x00\x00" + bytes([(n >> 21) & 0x7F, (n >> 14) & 0x7F, (n >> 7) & 0x7F, n & 0x7F]) + frame


@pytest.mark.parametrize("channels,depth", [(2, 24), (1, 16), (2, 20)])
def test_host_sink_writes_the_replaygain_fields(engine_lib, sink_probe, tmp_path, channels, depth):
    d = engine_lib
    if not os.path.exists(CLI):
        d.build_library()
    rate, S = 88200, 8820
    frames = 6 * S + 1234
    pcm = noise_pcm(frames, channels, depth, seed=5, dc=0.0, amp=0.05)
    (tmp_path / "x.pcm").write_bytes(pcm.tobytes())
    (tmp_path / "x.id3").write_bytes(id3_with_title("Song"))
    cells, io = measure(d, channels, depth, rate, pcm)
    r = integrated(d, channels, rate, cells, io)
    ref = R.integrate(R.cells(R.to_float(pcm, channels, depth), rate), rate, io.subblocks)
    assert abs(r.lufs - ref["lufs"]) <= 1e-6
    want = ["REPLAYGAIN_REFERENCE_LOUDNESS=-18.00 LUFS", "REPLAYGAIN_TRACK_GAIN=%+06.2f dB" % ref["gain_db"], "REPLAYGAIN_TRACK_PEAK=%.6f" % ref["peak"]]
    files = {}
    for name, on, step, tag in (("tagged", 1, 1 << 16, True), ("small_writes", 1, 1000, True), ("bare", 1, 1 << 20, False), ("off", 0, 1 << 16, True),
                                ("off_bare", 0, 1 << 16, False)):
        out = str(tmp_path / (name + ".flac"))
        args = [sink_probe, out, str(channels), str(depth), str(rate), str(on), str(tmp_path / "x.pcm"), str(step)] + ([str(tmp_path / "x.id3")] if tag else [])
        p = subprocess.run(args, capture_output=True, text=True)
        assert p.returncode == 0 and p.stdout == "ok\n", (p.stdout, p.stderr)
        files[name] = out
    assert vorbis_fields(files["tagged"]) == ["TITLE=Song"] + want
    assert vorbis_fields(files["bare"]) == want                          # the block is written even when the source has no tag
    assert open(files["small_writes"], "rb").read() == open(files["tagged"], "rb").read()
    assert vorbis_fields(files["off"]) == ["TITLE=Song"] and vorbis_fields(files["off_bare"]) is None
    for name in ("off", "off_bare"):                                     # without the switch: none of the fields, anywhere in the file
        assert b"REPLAYGAIN" not in open(files[name], "rb").read()
    # the audio is the same with and without the switch: the files differ in the comment block alone
    a, b = open(files["tagged"], "rb").read(), open(files["off"], "rb").read()
    assert len(a) - len(b) == sum(4 + len(w) for w in want) and a[-(len(b) - 100):] == b[-(len(b) - 100):]
    v = subprocess.run([CLI, "verify"] + [files[k] for k in ("tagged", "bare", "off")], capture_output=True, text=True)
    assert v.returncode == 0 and v.stdout.count(": ok\n") == 3, v.stdout


def test_host_sink_tags_silence_with_zero_gain(sink_probe, tmp_path):
    (tmp_path / "z.pcm").write_bytes(bytes(2 * 2 * 9000))
    out = str(tmp_path / "z.flac")
    p = subprocess.run([sink_probe, out, "2", "16", "8000", "1", str(tmp_path / "z.pcm"), "4096"], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout
    assert vorbis_fields(out) == ["REPLAYGAIN_REFERENCE_LOUDNESS=-18.00 LUFS", "REPLAYGAIN_TRACK_GAIN=+00.00 dB", "REPLAYGAIN_TRACK_PEAK=0.000000"]


def test_cli_refuses_replaygain_for_other_sinks(engine_lib, tmp_path):
    if not os.path.exists(CLI):
        engine_lib.build_library()
    for extra in (["-o", "w"], ["-o", "a", "--gpu-flac"], []):
        r = subprocess.run([CLI, "convert"] + extra + ["--replaygain", str(tmp_path / "x.dsf")], capture_output=True, text=True)
        assert r.returncode == 2 and r.stderr.startswith("ERROR:") and "--replaygain" in r.stderr and r.stderr.count("\n") == 1, (extra, r.stderr)
    r = subprocess.run([CLI, "convert", "-o", "f", "--loudness", str(tmp_path / "x.dsf")], capture_output=True, text=True)
    assert r.returncode == 2 and "--loudness" in r.stderr


# ---- the sanitised run ----

def test_host_twin_is_cut_invariant_sanitised(tmp_path):
    exe = str(tmp_path / "loud_fuzz")
    src = [os.path.join(ROOT, "tools", "loud_fuzz.cpp"), os.path.join(CSRC, "loud", "d2d_loud_host.cpp"), os.path.join(CSRC, "flac", "d2d_flac_host.cpp")]
    cmd = ["g++", "-g", "-O1", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe] + src
    r = subprocess.run(cmd, cwd=os.path.join(ROOT, "tools"), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    p = subprocess.run([exe, "1", "80"], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "fuzz ok" in p.stdout and not p.stderr, (p.stdout[-500:], p.stderr[-3000:])
