"""True peak, the host side (include/dsd2dxd_amd.h, "Loudness where the PCM is"): d2d_true_peak_measure_host -- the CPU twin of the GPU
call, built on dsd2dxd_amd/csrc/loud/true_peak.h, the source the kernel compiles too -- against tests/true_peak_ref.py, an independent
restatement in integers; the meter's d2d_loud_set_true_peak / _add_true_peaks / _true_peak; the FLAC sink's switch through
tools/loud_sink_probe.cpp; the CLI's refusal and line format; the refusals; a sanitised run of tools/true_peak_fuzz.cpp.  No GPU.
tests/test_gpu_true_peak.py holds the device call to this twin byte for byte.

Bounds.  Every double: exact, bit for bit -- the reference sums integers, and for float input follows the one fixed order of additions.
The fs/4 sine: the reference's value, which must lie in [0.98, 1.02] x amplitude while the sample peak is 0.70711 x amplitude.  The
worst-case streams: exactly (sum of |C[p]|) / 8192 x rail."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import true_peak_ref as T
from test_loudness_cpu import id3_with_title, vorbis_fields

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "dsd2dxd_amd", "dsd2dxd_amd_cli")
CSRC = os.path.join(ROOT, "dsd2dxd_amd", "csrc")
ERR_PARAM, ERR_CAPACITY, ERR_STATE = -1, -20, -40
DEPTHS = (16, 20, 24, 32)
CHANNELS = (1, 2, 3, 6, 8)
RATE, S = 8000, 800
MAGNITUDES = (11749, 16571, 16571, 11749)                               # the sums of |C[p]|


def noise_pcm(frames, channels, depth, seed):
    """packed frames of seeded noise over the whole range of the depth (floats: around +-0.5, some beyond full scale)"""
    rng = np.random.default_rng(seed)
    if depth == 32:
        return T.pack((0.5 * rng.standard_normal((frames, channels))).astype(np.float32), 32)
    full = 1 << ((20 if depth == 20 else depth) - 1)
    return T.pack(rng.integers(-full, full, (frames, channels)), depth)


def worst_case_pcm(phase, at, frames, depth, channels=1, channel=0):
    """a stream at the rail (+-(2^(bits-1) - 1), alternating) on one channel, silence on the others, whose twelve frames up to and
    including frame `at` follow the sign of C[phase], so that every product of y_phase(at) is positive: returns (pcm, the value there,
    exactly (sum of |C[phase]|) / 8192 x rail)"""
    bits = 20 if depth == 20 else depth
    hi, full = (1 << (bits - 1)) - 1, 1 << (bits - 1)
    x = np.zeros((frames, channels), dtype=np.int64)
    x[:, channel] = np.where(np.arange(frames) % 2 == 0, hi, -hi)
    for k in range(min(12, at + 1)):
        x[at - k, channel] = hi if T.COEF[phase, k] > 0 else -hi
    return T.pack(x, depth), MAGNITUDES[phase] * hi / 8192.0 / full      # (an integer under 2^53 over powers of two: exact)


def measure(d, channels, depth, rate, pcm, **kw):
    return d.true_peak_measure_host(channels, depth, rate, pcm, **kw)


def test_structure_has_the_public_layout(engine_lib):
    d = engine_lib
    assert C.sizeof(d.TruePeakIO) == 80
    assert (d.TruePeakIO.peaks.offset, d.TruePeakIO.subblocks.offset, d.TruePeakIO.peaks_out.offset, d.TruePeakIO.next_subblock.offset) == (40, 56, 64, 72)


def test_the_table_is_the_definition():
    assert [int(v) for v in T.COEF.sum(axis=1)] == [8205, 7971, 7971, 8205]
    assert tuple(int(v) for v in np.abs(T.COEF).sum(axis=1)) == MAGNITUDES
    h = np.zeros(48)
    for p in range(4):
        h[p::4] = T.COEF[p] / 8192.0
    f = np.abs(np.fft.rfft(h, 4096)) / 1.0                               # bin k is k / 4096 of the oversampled rate: fs is 1024 bins
    # flat up to 0.4 fs: nowhere further from 4.0 than at DC, where the four sums give 32352 / 8192 = 3.9492; under 0.041 from 0.6 fs on
    dc = 4.0 - 32352 / 8192.0
    assert f[0] == 32352 / 8192.0 and 0.050 < dc < 0.051
    assert np.all(np.abs(f[:int(0.4 * 1024) + 1] - 4.0) <= dc + 1e-12) and np.all(f[int(np.ceil(0.6 * 1024)):] < 0.041)


# ---- the twin against the reference ----

@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("channels", CHANNELS)
def test_host_twin_equals_the_reference_bit_for_bit(engine_lib, channels, depth):
    """3 sub-blocks and a partial fourth of seeded noise"""
    frames = 3 * S + S // 3
    pcm = noise_pcm(frames, channels, depth, seed=channels * 100 + depth)
    got, io = measure(engine_lib, channels, depth, RATE, pcm)
    assert (io.subblocks, io.peaks_out, io.next_subblock) == (3, 4 * channels, 3) and got.shape == (4, channels)
    want = T.cells(pcm, channels, depth, RATE)
    assert got.tobytes() == want.tobytes(), np.max(np.abs(got - want))
    # a call that is not final leaves the partial sub-block alone
    nf, io_nf = measure(engine_lib, channels, depth, RATE, pcm, final=False)
    assert (io_nf.subblocks, io_nf.peaks_out, io_nf.next_subblock) == (3, 3 * channels, 3) and nf.tobytes() == got[:3].tobytes()


def test_sine_at_a_quarter_of_the_rate_sampled_at_45_degrees(engine_lib):
    """every sample is +-0.70711 x amplitude; the oversampled signal reaches the amplitude"""
    amp = 2 ** 23 - 1
    n = np.arange(3 * S)
    x = np.round(amp * np.sin(np.pi / 2 * n + np.pi / 4)).astype(np.int64)
    pcm = T.pack(x[:, None], 24)
    got, io = measure(engine_lib, 1, 24, RATE, pcm)
    want = T.cells(pcm, 1, 24, RATE)
    a = amp / 2 ** 23
    print(f"fs/4 at 45 degrees: true peak {got.max() / a:.6f} x amplitude, sample peak {T.sample_peak(pcm, 1, 24) / a:.6f} x amplitude")
    assert got.tobytes() == want.tobytes()
    assert 0.98 * a <= got.max() <= 1.02 * a and abs(got.max() / a - 1.00956) < 1e-5
    assert abs(T.sample_peak(pcm, 1, 24) / a - 0.70711) < 1e-5


@pytest.mark.parametrize("depth", (16, 24))
@pytest.mark.parametrize("phase", range(4))
def test_worst_case_sums_are_exact_wherever_they_fall(engine_lib, phase, depth):
    """a rail-level stream whose twelve frames up to `at` follow the sign of C[phase]: y_phase(at) is sum |C[phase]| / 8192 x rail (about
    2^38 in units of a 24-bit step: what an int32 accumulator loses).  `at` is the first frame of a sub-block, the last frame of one,
    the last frame of a partial row, and frame 11 of the stream.  For the inner phases that is the largest value any stream within the
    rail can give, so it is the cell; the outer phases' pattern reads higher still through an inner phase, so there the reference's
    output at (at, phase) is held to the sum and the cell to the reference."""
    frames = 2 * S + 300
    for at, row in ((S, 1), (2 * S - 1, 1), (frames - 1, 2), (11, 0)):
        pcm, want = worst_case_pcm(phase, at, frames, depth, channels=2, channel=1)
        got, io = measure(engine_lib, 2, depth, RATE, pcm)
        assert got.tobytes() == T.cells(pcm, 2, depth, RATE).tobytes()
        assert T.outputs(pcm, 2, depth)[at, 1, phase] == want
        assert depth == 16 or want * 8192 * (1 << 23) > 2 ** 36             # (in steps: far beyond an int32)
        assert got[row, 1] >= want and np.all(got[:, 0] == 0.0)
        if phase in (1, 2):
            assert got[row, 1] == want == got.max(), (at, got, want)


def test_float_full_scale_reads_the_sum_of_magnitudes(engine_lib):
    """float input holds +-1.0 exactly: the inner phases read 16571 / 8192 = 2.0228, the largest reading of any input within full scale"""
    for phase in (1, 2):
        x = np.zeros((S + 20, 1), dtype=np.float32)
        x[S - 11:S + 1, 0] = np.sign(T.COEF[phase][::-1])                # x[S - k] = sign(C[phase][k]): the first frame of sub-block 1
        got, io = measure(engine_lib, 1, 32, RATE, T.pack(x, 32))
        assert got[1, 0] == MAGNITUDES[phase] / 8192.0 == got.max() and 2.02 < got[1, 0] <= 2.03


@pytest.mark.parametrize("frames", (1, 11, 12))
def test_streams_of_a_few_frames(engine_lib, frames):
    for channels, depth in ((1, 16), (2, 24), (3, 32)):
        pcm = noise_pcm(frames, channels, depth, seed=frames)
        got, io = measure(engine_lib, channels, depth, RATE, pcm)
        assert (io.subblocks, io.peaks_out, io.next_subblock) == (0, channels, 0)
        assert got.tobytes() == T.cells(pcm, channels, depth, RATE).tobytes()
        nf, io_nf = measure(engine_lib, channels, depth, RATE, pcm, final=False)
        assert io_nf.peaks_out == 0


@pytest.mark.parametrize("channels,depth,rate", [(2, 24, 8000), (3, 16, 8010), (1, 32, 8000), (6, 20, 11020)])
def test_cutting_with_exactly_eleven_frames_of_history_gives_the_same_bytes(engine_lib, channels, depth, rate):
    s = rate // 10
    frames = 5 * s + 17
    pcm = noise_pcm(frames, channels, depth, seed=7)
    fb = channels * T.sample_bytes(depth)
    whole, io = measure(engine_lib, channels, depth, rate, pcm)
    assert io.peaks_out == 6 * channels
    for ends in ([s * k for k in range(1, 6)] + [frames], [2 * s, 4 * s, frames], [5, s - 1, s + 1, 3 * s + 9, 3 * s + 9, 4 * s, frames - 1, frames]):
        got, nxt = [], 0
        for end in ends:
            first = max(0, nxt * s - 11)
            piece = pcm[first * fb:end * fb]
            if piece.size == 0:
                continue
            peaks, cio = measure(engine_lib, channels, depth, rate, piece, first_frame=first, first_subblock=nxt, final=end == frames)
            assert cio.next_subblock == end // s and cio.subblocks == end // s - nxt
            got.append(peaks)
            nxt = cio.next_subblock
        assert np.concatenate(got).tobytes() == whole.tobytes(), ends


# ---- refusals ----

def test_refusals_return_their_codes_and_write_nothing(engine_lib):
    d = engine_lib
    L = d.lib()
    pcm = noise_pcm(4 * S, 2, 16, seed=1)
    peaks = np.full(16, 7.5, dtype=np.float64)

    def io(**kw):
        v = dict(pcm=pcm.ctypes.data, frames=4 * S, first_frame=0, first_subblock=0, final=1, peaks=peaks.ctypes.data, peaks_capacity=16)
        v.update(kw)
        return d.TruePeakIO(v["pcm"], v["frames"], v["first_frame"], v["first_subblock"], v["final"], 0, v["peaks"], v["peaks_capacity"], 111, 222, 333)

    cases = [((2, 17, 8000), {}, ERR_PARAM, "bit depth"), ((2, 12, 8000), {}, ERR_PARAM, "bit depth"),
             ((0, 16, 8000), {}, ERR_PARAM, "channel"), ((9, 16, 8000), {}, ERR_PARAM, "channel"),
             ((2, 16, 8005), {}, ERR_PARAM, "rate"), ((2, 16, 7990), {}, ERR_PARAM, "rate"), ((2, 16, 1411210), {}, ERR_PARAM, "rate"),
             ((2, 16, 8000), dict(pcm=None), ERR_PARAM, "non-null"), ((2, 16, 8000), dict(peaks=None), ERR_PARAM, "non-null"),
             ((2, 16, 8000), dict(first_subblock=0, first_frame=1), ERR_PARAM, "history"),
             # one frame too few: sub-block 1 needs frame 789
             ((2, 16, 8000), dict(first_subblock=1, first_frame=S - 10, frames=3 * S), ERR_PARAM, "history"),
             ((2, 16, 8000), dict(first_subblock=3, first_frame=3 * S, frames=S), ERR_PARAM, "history"),
             ((2, 16, 8000), dict(peaks_capacity=7), ERR_CAPACITY, "peaks_capacity")]
    for (ch, depth, rate), kw, code, text in cases:
        rec = io(**kw)
        rc = L.d2d_true_peak_measure_host(ch, depth, rate, C.byref(rec))
        assert rc == code and text in L.d2d_flac_error().decode(), ((ch, depth, rate), kw, rc, L.d2d_flac_error())
        assert (rec.subblocks, rec.peaks_out, rec.next_subblock) == (111, 222, 333) and np.all(peaks == 7.5)
    assert L.d2d_true_peak_measure_host(2, 16, 8000, None) == ERR_PARAM
    # exactly eleven frames of history pass; the call with the capacity it needs writes exactly its 8 doubles
    rec = io(first_subblock=1, first_frame=S - 11, frames=3 * S + 11, pcm=pcm.ctypes.data + (S - 11) * 4)
    assert L.d2d_true_peak_measure_host(2, 16, 8000, C.byref(rec)) == 0 and (rec.subblocks, rec.peaks_out, rec.next_subblock) == (3, 6, 4)
    assert peaks[:6].tobytes() == T.cells(pcm, 2, 16, 8000)[1:4].tobytes()
    peaks[:] = 7.5
    rec = io(peaks_capacity=8)
    assert L.d2d_true_peak_measure_host(2, 16, 8000, C.byref(rec)) == 0 and rec.peaks_out == 8 and np.all(peaks[8:] == 7.5) and np.all(peaks[:8] != 7.5)
    # frames == 0 leaves the record alone
    rec = io(frames=0, pcm=None, peaks=None)
    assert L.d2d_true_peak_measure_host(2, 16, 8000, C.byref(rec)) == 0 and (rec.subblocks, rec.peaks_out, rec.next_subblock) == (111, 222, 333)
    # the device call checks before it touches a device: the same refusals without a GPU, misalignment among them
    rec = io(peaks_capacity=7)
    assert L.d2d_true_peak_measure_device(2, 16, 8000, C.byref(rec), 1, None) == ERR_CAPACITY and rec.peaks_out == 222
    rec = io(pcm=(pcm.ctypes.data | 15) + 1 + 8)
    assert L.d2d_true_peak_measure_device(2, 16, 8000, C.byref(rec), 1, None) == ERR_PARAM and "aligned" in L.d2d_flac_error().decode()
    rec = io(peaks=peaks.ctypes.data + 4)
    assert L.d2d_true_peak_measure_device(2, 16, 8000, C.byref(rec), 1, None) == ERR_PARAM and "aligned" in L.d2d_flac_error().decode()
    assert L.d2d_true_peak_measure_device(2, 16, 8000, None, 1, None) == ERR_PARAM and L.d2d_true_peak_measure_device(2, 16, 8000, None, 0, None) == 0
    assert np.all(peaks[8:] == 7.5)


# ---- the meter ----

def test_meter_reports_the_larger_of_sample_peak_and_true_peak(engine_lib):
    d = engine_lib
    ch = 2
    pcm = noise_pcm(3 * S + 100, ch, 24, seed=4)
    cells, lio = d.loud_measure_host(ch, 24, RATE, pcm)
    peaks, pio = measure(d, ch, 24, RATE, pcm)
    plain = d.LoudMeter(ch, RATE)
    plain.add(cells, has_partial=True)
    before = plain.finish()
    m = d.LoudMeter(ch, RATE, true_peak=True)
    m.add(cells, has_partial=True)
    with pytest.raises(d.D2DError) as ei:                                # after an add the switch is fixed
        m.set_true_peak(False)
    assert ei.value.code == ERR_PARAM
    with pytest.raises(d.D2DError) as ei:                                # no true-peak rows yet
        m.true_peak()
    assert ei.value.code == ERR_PARAM
    m.add_true_peaks(peaks[:2])                                          # two whole rows, in two calls, independently of add()
    with pytest.raises(d.D2DError) as ei:                                # 2 rows against 3 and a partial one
        m.true_peak()
    assert ei.value.code == ERR_PARAM
    m.add_true_peaks(peaks[2:3])
    with pytest.raises(d.D2DError):                                      # the partial row is still missing
        m.true_peak()
    m.add_true_peaks(peaks[3:], has_partial=True)
    r = m.finish()
    assert bytes(r) == bytes(before), "d2d_loud_finish does not change with the switch"
    assert m.true_peak() == max(r.peak, peaks.max()) and peaks.max() > r.peak
    with pytest.raises(d.D2DError) as ei:                                # nothing comes behind the partial row
        m.add_true_peaks(peaks[:1])
    assert ei.value.code == ERR_STATE
    # a meter that was not switched on: refuses rows and has no true peak; its result is what it was
    with pytest.raises(d.D2DError) as ei:
        plain.add_true_peaks(peaks, has_partial=True)
    assert ei.value.code == ERR_PARAM
    with pytest.raises(d.D2DError):
        plain.true_peak()
    assert bytes(plain.finish()) == bytes(before)
    # never below the sample peak: the last frame of a stream is seen by one tap only (the eleven outputs behind it are dropped)
    x = np.zeros((S + 5, 1), dtype=np.int64)
    x[-1, 0] = 2 ** 23 - 1
    one = T.pack(x, 24)
    c1, _ = d.loud_measure_host(1, 24, RATE, one)
    p1, _ = measure(d, 1, 24, RATE, one)
    m1 = d.LoudMeter(1, RATE, true_peak=True)
    m1.add(c1, has_partial=True)
    m1.add_true_peaks(p1, has_partial=True)
    assert p1.max() < 0.04 and m1.true_peak() == m1.finish().peak == (2 ** 23 - 1) / 2 ** 23
    # the switch may be moved before the first add, and null arguments are refused
    m2 = d.LoudMeter(1, RATE)
    for on in (True, False, True):
        m2.set_true_peak(on)
    m2.add_true_peaks(p1, has_partial=True)
    with pytest.raises(d.D2DError):
        m2.set_true_peak(False)
    L = d.lib()
    assert L.d2d_loud_set_true_peak(None, 1) == ERR_PARAM and L.d2d_loud_add_true_peaks(None, None, 0, 0) == ERR_PARAM
    assert L.d2d_loud_true_peak(None, None) == ERR_PARAM and L.d2d_loud_true_peak(m1._h, None) == ERR_PARAM
    assert L.d2d_loud_add_true_peaks(m2._h, None, 1, 0) == ERR_PARAM
    for x in (plain, m, m1, m2):
        x.close()


# ---- files and the command line ----

@pytest.fixture(scope="module")
def sink_probe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("tpeak") / "loud_sink_probe")
    src = [os.path.join(ROOT, "tools", "loud_sink_probe.cpp"), os.path.join(CSRC, "host", "pcm_sink.cpp"), os.path.join(CSRC, "host", "id3_tag.cpp"),
           os.path.join(CSRC, "loud", "d2d_loud_host.cpp"), os.path.join(CSRC, "flac", "d2d_flac_host.cpp")]
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-o", exe] + src + ["-lpthread"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


@pytest.mark.parametrize("channels,depth", [(2, 24), (1, 16)])
def test_host_sink_writes_the_true_peak_as_track_peak(engine_lib, sink_probe, tmp_path, channels, depth):
    d = engine_lib
    if not os.path.exists(CLI):
        d.build_library()
    rate, s = 88200, 8820
    frames = 3 * s + 1234
    pcm = noise_pcm(frames, channels, depth, seed=5)
    (tmp_path / "x.pcm").write_bytes(pcm.tobytes())
    (tmp_path / "x.id3").write_bytes(id3_with_title("Song"))
    want = max(T.cells(pcm, channels, depth, rate).max(), T.sample_peak(pcm, channels, depth))
    assert want > 1.0, "the noise overshoots: the field must hold a value above 1"
    files = {}
    for name, mode, step in (("true", 2, 1 << 16), ("small_writes", 2, 1000), ("sample", 1, 1 << 16), ("off", 0, 1 << 16)):
        out = str(tmp_path / (name + ".flac"))
        p = subprocess.run([sink_probe, out, str(channels), str(depth), str(rate), str(mode), str(tmp_path / "x.pcm"), str(step), str(tmp_path / "x.id3")],
                           capture_output=True, text=True)
        assert p.returncode == 0 and p.stdout == "ok\n", (p.stdout, p.stderr)
        files[name] = open(out, "rb").read()
    fields, sample = vorbis_fields(str(tmp_path / "true.flac")), vorbis_fields(str(tmp_path / "sample.flac"))
    assert fields[-1] == "REPLAYGAIN_TRACK_PEAK=%.6f" % want and sample[-1] == "REPLAYGAIN_TRACK_PEAK=%.6f" % T.sample_peak(pcm, channels, depth)
    assert fields[:-1] == sample[:-1] and fields[0] == "TITLE=Song"
    assert files["small_writes"] == files["true"]
    # the switch moves the eight characters of the value and nothing else
    diff = [i for i in range(len(files["true"])) if files["true"][i] != files["sample"][i]]
    assert len(files["true"]) == len(files["sample"]) and diff and max(diff) - min(diff) < 8
    assert b"REPLAYGAIN" not in files["off"]
    v = subprocess.run([CLI, "verify", str(tmp_path / "true.flac")], capture_output=True, text=True)
    assert v.returncode == 0 and v.stdout.count(": ok\n") == 1, v.stdout
    # without `replaygain` the sink refuses the switch
    p = subprocess.run([sink_probe, str(tmp_path / "no.flac"), str(channels), str(depth), str(rate), "3", str(tmp_path / "x.pcm"), "4096"], capture_output=True, text=True)
    assert p.returncode == 1 and "ReplayGain" in p.stdout


def test_placeholder_holds_the_filters_worst_case(sink_probe, tmp_path):
    """the largest reading of any input within full scale is 16571 / 8192 = 2.0228: the same eight characters as 0.000000"""
    x = np.zeros((9000, 1), dtype=np.int64)
    x[5000 - 11:5000 + 1, 0] = np.where(T.COEF[1][::-1] < 0, -(1 << 15), (1 << 15) - 1)
    (tmp_path / "w.pcm").write_bytes(T.pack(x, 16).tobytes())
    out = str(tmp_path / "w.flac")
    p = subprocess.run([sink_probe, out, "1", "16", "8000", "2", str(tmp_path / "w.pcm"), "4096"], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout
    want = T.cells(T.pack(x, 16), 1, 16, 8000).max()
    assert 2.02 < want <= 2.03 and vorbis_fields(out)[-1] == "REPLAYGAIN_TRACK_PEAK=%.6f" % want
    assert len("%.6f" % want) == len("0.000000")


def test_cli_refuses_true_peak_without_replaygain_on_convert(engine_lib, tmp_path):
    if not os.path.exists(CLI):
        engine_lib.build_library()
    for extra in (["-o", "f"], ["-o", "f", "--gpu-flac"], ["-o", "w"], []):
        r = subprocess.run([CLI, "convert"] + extra + ["--true-peak", str(tmp_path / "x.dsf")], capture_output=True, text=True)
        assert r.returncode == 2 and r.stderr.startswith("ERROR:") and "--true-peak" in r.stderr and "--replaygain" in r.stderr and r.stderr.count("\n") == 1, (extra, r.stderr)
    # with --replaygain the pair is still a FLAC matter
    r = subprocess.run([CLI, "convert", "-o", "w", "--replaygain", "--true-peak", str(tmp_path / "x.dsf")], capture_output=True, text=True)
    assert r.returncode == 2 and "--replaygain" in r.stderr


# ---- the sanitised run ----

def test_host_twin_against_a_naive_loop_sanitised(tmp_path):
    exe = str(tmp_path / "true_peak_fuzz")
    src = [os.path.join(ROOT, "tools", "true_peak_fuzz.cpp"), os.path.join(CSRC, "loud", "d2d_loud_host.cpp"), os.path.join(CSRC, "flac", "d2d_flac_host.cpp")]
    cmd = ["g++", "-g", "-O1", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe] + src
    r = subprocess.run(cmd, cwd=os.path.join(ROOT, "tools"), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    p = subprocess.run([exe, "1", "60"], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "fuzz ok" in p.stdout and not p.stderr, (p.stdout[-500:], p.stderr[-3000:])
