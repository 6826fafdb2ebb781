"""d2d_convert_streams_flac (include/dsd2dxd_amd.h, "The batch driver") through the C ABI: five streams of different lengths in
lockstep through one engine of five files, against d2d_convert_stream_flac_loud on each stream alone on an engine of one file at the
default chunk.  Everything is compared for equality: the frame bytes, stats, check, md5, every field of d2d_loud_result and the true
peak.  Lengths per channel: nothing; 4096 bytes (only a short final block); 37 and 150 x 4096 (more than one loudness sub-block, not a
whole number of FLAC blocks); 64 x 4096, which ends exactly on a chunk edge of the batch's 8 x 4096 chunk."""
import pytest

from helpers import pack_layout, synth

gpu = pytest.mark.gpu
ERR_IO = -50
BLOCK = 4096
LENGTHS = (0, BLOCK, 37 * BLOCK, 150 * BLOCK, 64 * BLOCK)
CHUNK = 8 * BLOCK
ENGINES = {
    "dsd64-88k2-stereo-24-planar-lsb": dict(dsd_rate=1, output_rate=88200, channels=2, fmt="P", endianness="L", block_size=4096, filter="E",
                                            bit_depth=24, dither="T", seed=7),
    "dsd64-96k-mono-16": dict(dsd_rate=1, output_rate=96000, channels=1, fmt="I", endianness="M", block_size=1, filter="E",
                              bit_depth=16, dither="T", seed=8),
    "dsd128-176k4-six-20-interleaved-msb": dict(dsd_rate=2, output_rate=176400, channels=6, fmt="I", endianness="M", block_size=1, filter="E",
                                                bit_depth=20, dither="T", seed=9),
}
_streams = {}


def streams(name):
    """the five streams of an engine, in its layout, computed once"""
    if name not in _streams:
        kw = ENGINES[name]
        ch, msb = kw["channels"], kw["endianness"] == "M"
        out = []
        for f, n in enumerate(LENGTHS):
            chans = [synth("sine" if (f + c) % 2 == 0 else "pink", n, seed=10 * f + c + 1, amp=0.3 if (f + c) % 2 == 0 else 0.098,
                           freq=400.0 + 300.0 * c + 50.0 * f, dsd_rate=kw["dsd_rate"], msb_first=msb) for c in range(ch)]
            out.append(pack_layout(chans, kw["fmt"], kw["block_size"]).tobytes() if n else b"")
        _streams[name] = out
    return _streams[name]


def reader(data, ch, fail=False):
    """reads whole chunks of `cap` bytes per channel (whole planar blocks: cap is a multiple of the block size)"""
    pos = [0]

    def read(cap):
        if fail:
            return None
        a = pos[0]
        pos[0] = min(len(data), a + cap * ch)
        return data[a:pos[0]]
    return read


def meter_outcome(d, m):
    r = m.finish()
    try:
        tp = m.true_peak()
    except d.D2DError as ex:                                        # a stream without a frame has no rows
        tp = ("refused", ex.code)
    return bytes(r), tp


def alone(d, kw, data, effort):
    """d2d_convert_stream_flac_loud for one stream on an engine of one file at the default chunk, everything switched on"""
    rate, ch = kw["output_rate"], kw["channels"]
    e, m, out = d.Engine(**kw), d.LoudMeter(ch, rate, true_peak=True), []
    stats, chk, md5 = e.convert_stream_flac(reader(data, ch), out.append, total_bytes_per_channel=len(data) // ch, effort=effort,
                                            verify=True, md5=True, loud=m)
    e.close()
    res = (b"".join(out), (stats.samples_per_channel, stats.blocks, stats.min_frame_bytes, stats.max_frame_bytes), chk.as_tuple(), md5) + meter_outcome(d, m)
    m.close()
    return res


def together(d, kw, datas, effort, chunk=CHUNK, fail=None):
    rate, ch, n = kw["output_rate"], kw["channels"], len(datas)
    e = d.Engine(n_files=n, **kw)
    meters, outs = [d.LoudMeter(ch, rate, true_peak=True) for _ in range(n)], [[] for _ in range(n)]
    try:
        r = e.convert_streams_flac([reader(x, ch, fail == f) for f, x in enumerate(datas)], [o.append for o in outs],
                                   totals=[len(x) // ch for x in datas], chunk_bytes_per_channel=chunk, effort=effort, verify=True, md5=True,
                                   louds=meters)
    finally:
        e.close()
    res = []
    for f in range(n):
        s = r["stats"][f]
        res.append((b"".join(outs[f]), (s.samples_per_channel, s.blocks, s.min_frame_bytes, s.max_frame_bytes), r["checks"][f].as_tuple(),
                    r["md5"][f]) + meter_outcome(d, meters[f]))
        meters[f].close()
    return res, r


@gpu
@pytest.mark.parametrize("effort", (0, 12))
@pytest.mark.parametrize("name", ENGINES)
def test_every_file_of_the_batch_equals_its_stream_alone(engine_lib, name, effort):
    d, kw, datas = engine_lib, ENGINES[name], streams(name)
    got, r = together(d, kw, datas, effort)
    for f, data in enumerate(datas):
        want = alone(d, kw, data, effort)
        what = ("frame bytes", "stats", "check", "md5", "loudness result", "true peak")
        for k in range(len(what)):
            assert got[f][k] == want[k], f"file {f}: {what[k]} differ" + ("" if k == 0 else f": {got[f][k]} != {want[k]}")
    # the streams did something: whole and short blocks, a verified record per block, no write call for the empty stream
    assert got[0][0] == b"" and got[0][1] == (0, 0, 0, 0) and all(g[1][1] > 0 and g[2][1] == g[1][1] and g[2][2] == 0 for g in got[1:])
    assert r["chunks"] == 150 // 8 + 1


@gpu
def test_a_failing_read_names_its_file(engine_lib):
    d, name = engine_lib, "dsd64-96k-mono-16"
    with pytest.raises(d.D2DError) as ex:
        together(d, ENGINES[name], streams(name), 0, fail=2)
    assert ex.value.code == ERR_IO and "file 2" in ex.value.message, ex.value.message


@gpu
def test_device_calls_per_chunk_do_not_depend_on_the_file_count(engine_lib):
    """the driver's own count of what it enqueued (d2d_streams_options.device_calls): ten calls a chunk -- upload, translate, MD5, the
    segment move, loudness, true peak, encode, verify, the pack, the synchronise -- and three around the hash, for one file or for five"""
    d, name = engine_lib, "dsd64-88k2-stereo-24-planar-lsb"
    kw, datas = ENGINES[name], streams(name)
    _, one = together(d, kw, [datas[3]], 0)
    _, five = together(d, kw, datas, 0)
    assert one["chunks"] == five["chunks"] == 19
    assert one["device_calls"] == five["device_calls"] == 10 * 19 + 3


@gpu
def test_parameter_errors_come_before_any_device_call(engine_lib):
    d, name = engine_lib, "dsd64-96k-mono-16"
    kw, datas = ENGINES[name], streams(name)
    with pytest.raises(d.D2DError) as ex:                                  # three streams into an engine of five files
        e = d.Engine(n_files=5, **kw)
        try:
            e.convert_streams_flac([reader(x, 1) for x in datas[:3]], [None] * 3)
        finally:
            e.close()
    assert ex.value.code == -1 and "file count" in ex.value.message
    with pytest.raises(d.D2DError) as ex:                                  # a meter of another rate than the one before it
        e = d.Engine(n_files=2, **kw)
        try:
            e.convert_streams_flac([reader(x, 1) for x in datas[:2]], [None] * 2, louds=[d.LoudMeter(1, 96000), d.LoudMeter(1, 48000)])
        finally:
            e.close()
    assert ex.value.code == -1 and "file 1" in ex.value.message
