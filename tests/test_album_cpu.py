"""Album loudness on the host (include/dsd2dxd_amd.h, "Album loudness"): d2d_loud_finish_album and d2d_loud_true_peak_album.

The reference is a numpy restatement of the two gates over the CONCATENATED block powers of the tracks -- blocks do not span tracks --
with the cells of tests/loudness_ref.py.  Bound: 1e-6 LU, the one tests/test_loudness_cpu.py holds d2d_loud_finish to against
loudness_ref.integrate; counts and peaks exact."""
import numpy as np
import pytest

import loudness_ref as R

ERR_PARAM = -1
RATE, CH = 8000, 2
LUFS_TOL = 1e-6


def sine_track(dbfs, seconds, f=997.0):
    n = int(RATE * seconds)
    x = np.round(np.sin(2 * np.pi * f * np.arange(n) / RATE) * 10 ** (dbfs / 20) * 2 ** 23).astype(np.int64)
    return R.pack(np.repeat(x[:, None], CH, axis=1), 24)


def silent_track(seconds):
    return np.zeros(int(RATE * seconds) * CH * 3, dtype=np.uint8)


def meter_of(d, pcm, true_peak=False, channels=CH, rate=RATE, weights=None):
    """a finished-with-adding meter of the host twins' cells (and true-peak rows) of one track"""
    m = d.LoudMeter(channels, rate, weights, true_peak=true_peak)
    cells, io = d.loud_measure_host(channels, 24, rate, pcm)
    partial = io.cells_out > io.subblocks * channels
    m.add(cells, has_partial=partial)
    if true_peak:
        peaks, _ = d.true_peak_measure_host(channels, 24, rate, pcm)
        m.add_true_peaks(peaks, has_partial=partial)
    return m


def block_powers(pcm):
    """sum_c G_c z_c of every 400 ms block of one track, from the reference's cells; and its sample peak"""
    c = R.cells(R.to_float(pcm, CH, 24), RATE)
    whole = (len(pcm) // (CH * 3)) // (RATE // 10)
    e = c[:whole, :, 0]
    S = RATE // 10
    power = np.array([np.sum(e[b:b + 4].sum(axis=0) / (4.0 * S)) for b in range(max(0, whole - 3))])
    return power, (float(c[:, :, 1].max()) if c.size else 0.0)


def album_reference(tracks):
    got = [block_powers(t) for t in tracks]
    power = np.concatenate([p for p, _ in got]) if got else np.zeros(0)
    peak = max(pk for _, pk in got)
    with np.errstate(divide="ignore"):
        l = -0.691 + 10.0 * np.log10(power)
    above = l > -70.0
    res = dict(lufs=None, gain_db=0.0, peak=peak, blocks_total=power.size, removed_absolute=int(power.size - above.sum()), removed_relative=0)
    if above.any():
        rel = -0.691 + 10.0 * np.log10(power[above].mean()) - 10.0
        keep = above & (l > rel)
        res["removed_relative"] = int(above.sum() - keep.sum())
        res["kept"] = int(keep.sum())
        res["lufs"] = float(-0.691 + 10.0 * np.log10(power[keep].mean()))
        res["gain_db"] = -18.0 - res["lufs"]
    return res


TWO_SINES = lambda: [sine_track(-20.0, 4.0), sine_track(-32.0, 2.0)]            # noqa: E731  (the louder one is longer: the mean lies 1.6 dB under it, the gate 11.6 dB)


@pytest.mark.parametrize("case", ["two_sines", "with_silence"])
def test_album_gates_against_the_concatenated_reference(engine_lib, case):
    d = engine_lib
    tracks = TWO_SINES() + ([silent_track(2.0)] if case == "with_silence" else [])
    ref = album_reference(tracks)
    # a test in which no gate fires shows nothing: the quieter sine's blocks go, the louder one's stay, the silence goes whole
    assert ref["removed_relative"] > 0 and ref["kept"] > 0, ref
    if case == "with_silence":
        assert ref["removed_absolute"] == 2 * 10 - 3, ref
    meters = [meter_of(d, t) for t in tracks]
    r = d.loud_finish_album(meters)
    print(f"{case}: {r.lufs:.9f} LUFS, reference {ref['lufs']:.9f}; gates removed {ref['removed_absolute']} + {ref['removed_relative']} of {ref['blocks_total']}")
    assert r.valid == 1 and abs(r.lufs - ref["lufs"]) <= LUFS_TOL
    assert abs(r.gain_db - ref["gain_db"]) <= LUFS_TOL and r.gain_db == -18.0 - r.lufs
    assert r.blocks_total == ref["blocks_total"] and r.blocks_gated == ref["removed_absolute"] + ref["removed_relative"]
    assert r.peak == ref["peak"] == max(m.finish().peak for m in meters)
    # the order of the meters decides the order of the sums only
    assert abs(d.loud_finish_album(meters[::-1]).lufs - r.lufs) <= LUFS_TOL
    for m in meters:
        m.close()


def test_album_of_silence_is_invalid(engine_lib):
    d = engine_lib
    meters = [meter_of(d, silent_track(1.0)), meter_of(d, silent_track(2.0))]
    r = d.loud_finish_album(meters)
    assert (r.valid, r.lufs, r.gain_db, r.peak) == (0, 0.0, 0.0, 0.0)
    assert r.blocks_total == r.blocks_gated == (10 - 3) + (20 - 3)


def test_one_meter_is_d2d_loud_finish_bit_for_bit(engine_lib):
    d = engine_lib
    rng = np.random.default_rng(5)
    x = np.concatenate([0.2 * rng.standard_normal((2 * RATE, CH)), 0.004 * rng.standard_normal((RATE, CH)), np.zeros((RATE, CH))])
    pcm = R.pack(np.round(x * 2 ** 23).clip(-2 ** 23, 2 ** 23 - 1).astype(np.int64), 24)
    m = meter_of(d, pcm, true_peak=True)
    a, b = d.loud_finish_album([m]), m.finish()
    assert bytes(a) == bytes(b) and a.valid == 1 and a.blocks_gated > 0
    assert d.loud_true_peak_album([m]) == m.true_peak()


def test_album_true_peak_is_the_largest(engine_lib):
    d = engine_lib
    meters = [meter_of(d, t, true_peak=True) for t in TWO_SINES()]
    want = max(m.true_peak() for m in meters)
    assert d.loud_true_peak_album(meters) == want == meters[0].true_peak() > meters[1].true_peak()
    # under d2d_loud_true_peak's conditions for each meter: one without true-peak rows is refused
    with pytest.raises(d.D2DError) as ex:
        d.loud_true_peak_album([meters[0], meter_of(d, silent_track(0.5))])
    assert ex.value.code == ERR_PARAM


def test_mismatched_meters_and_empty_albums_are_refused(engine_lib):
    d = engine_lib
    base = meter_of(d, sine_track(-20.0, 1.0))
    mono = d.LoudMeter(1, RATE)
    other_rate = d.LoudMeter(CH, 48000)
    other_weights = d.LoudMeter(CH, RATE, [1.0, 0.5])
    for bad in ([base, mono], [base, other_rate], [base, other_weights], [], [base, None]):
        with pytest.raises(d.D2DError) as ex:
            d.loud_finish_album(bad)
        assert ex.value.code == ERR_PARAM, bad
        with pytest.raises(d.D2DError) as ex:
            d.loud_true_peak_album(bad)
        assert ex.value.code == ERR_PARAM, bad
    assert d.loud_finish_album([base, d.LoudMeter(CH, RATE, [1.0, 1.0])]).valid == 1        # the default weights, spelled out
