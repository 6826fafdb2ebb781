"""GPU tests of the engine's growing buffers where state is carried across the reallocation: the cascade's scratch with its
stage-A history, the noise shaper's f64 line next to it, and the staging of d2d_translate_batch_host between two calls."""
import numpy as np
import pytest

from helpers import pack_layout, random_bytes

pytestmark = pytest.mark.gpu

KW = dict(channels=2, fmt="P", endianness="L", block_size=4096, filter="E", bit_depth=24, seed=77)


def _cascade_regrowth(engine_lib, oracle_mod, dither):
    """DSD256 -> 96 kHz: the second call's 5120 stage-A outputs outgrow the 4096-sample scratch line that already carries the first call's
    P = 96 samples in front (dither N: 1393 + 8 outputs also outgrow the 1024-sample f64 line of the first call, shaper state carried)"""
    kw = dict(KW, dsd_rate=4, output_rate=96000, dither=dither)
    e = engine_lib.Engine(kernel=2, **kw)
    o = oracle_mod.Oracle(**kw)
    assert e.info()["P"] == 96
    for i, (n, frames) in enumerate([(4096, 279), (20480, 1393), (4096, 279)]):
        buf = pack_layout([random_bytes(n, 900 + i), random_bytes(n, 910 + i)], "P", 4096)
        g, gf = e.translate(buf)
        r, rf = o.translate(buf)
        assert gf == rf == frames, (i, gf, rf)
        assert np.array_equal(g, r[:rf * e.frame_bytes]), i
    assert [e.peak(c) for c in range(2)] == [o.peak(c) for c in range(2)]
    e.close()


def _host_staging_regrowth(engine_lib, oracle_mod, dither):
    """two files through the staged pipeline of d2d_translate_batch_host, first in 4096-byte slices, then the rest of each file in
    16384-byte slices on the same engine: all four staging buffers grow between the calls, the files' state is carried"""
    kw = dict(KW, dsd_rate=1, output_rate=88200, dither=dither)
    first, rest = [8192, 12288], [40960, 20480]
    chans = [[random_bytes(a + b, 920 + 2 * i + c) for c in range(2)] for i, (a, b) in enumerate(zip(first, rest))]
    e = engine_lib.Engine(n_files=2, kernel=2, debug=engine_lib.DBG_HOST_STAGED, **kw)
    fb = e.frame_bytes
    got = [[], []]
    for lens, starts, slice_bytes in ((first, [0, 0], 4096), (rest, first, 16384)):
        ins = [pack_layout([ch[s0:s0 + n] for ch in chans[i]], "P", 4096) for i, (n, s0) in enumerate(zip(lens, starts))]
        outs = [np.zeros(e.next_frames(n, file=i) * fb + 64, dtype=np.uint8) for i, n in enumerate(lens)]
        ios = (engine_lib.FileIO * 2)()
        for i, n in enumerate(lens):
            ios[i].dsd = ins[i].ctypes.data; ios[i].bytes_per_channel = n
            ios[i].pcm = outs[i].ctypes.data; ios[i].pcm_capacity_bytes = outs[i].size
        e.translate_batch_host(ios, slice_bytes)
        for i in range(2):
            got[i].append(outs[i][:ios[i].frames_out * fb].copy())
    for i in range(2):
        r, rf = oracle_mod.Oracle(**kw).translate(pack_layout(chans[i], "P", 4096))
        assert np.array_equal(np.concatenate(got[i]), r[:rf * fb]), i
    e.close()


@pytest.mark.parametrize("case,dither", [(_cascade_regrowth, "T"), (_cascade_regrowth, "N"), (_host_staging_regrowth, "T")],
                         ids=["cascade_scratch", "cascade_scratch_and_ys", "host_batch_staging"])
def test_buffers_regrow_with_carried_state(engine_lib, oracle_mod, case, dither):
    case(engine_lib, oracle_mod, dither)
