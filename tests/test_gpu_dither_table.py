"""A call whose files all stand at the same output index hashes its dither words once, into a table, and the resident dithered flavours of the
fp6 kernel's integer requantiser (M = 32, stereo frames at 0 dB, 16 or 24 bits) read them there instead of hashing them file by file (DESIGN.md
4.0, d2d_engine.cpp: dither_table_serves, d2d_mx_kernel.h: DT).  A tile is 576 outputs = 2304 bytes per channel.

Every case runs the same calls on two engines, one of them under D2D_DBG_NO_DITHER_TABLE, and on the oracle: the frames of every call and file
are compared with np.array_equal, the peaks with ==, and d2d_dither_table_calls says after every call which route it took.
  * calls shorter than a tile, of one tile, one tile + 1, 3 tiles + 5 in two ragged calls (the second call's table starts at a non-zero index);
  * every instantiation that reads the table on the E filter (24 and 16 bits, T and R), one format on the X and C filters, byte-interleaved
    stereo, a batch whose waves walk several tiles each; and the dithered formats of the f64 requantiser (20 bits, -3 dB at 24 and 16 bits T and
    R, float frames with the F dither), which were measured no faster with the table and stay off it: the same batches, the route asserted off;
  * files of different length in one batch, one of which ends in the first call and feeds nothing afterwards;
  * calls the table does not serve: one file moved ahead with d2d_seek, one file fewer than the threshold;
  * tiles that take the careful path next to tiles that read the table: exact ties, both rails (tests/adversarial.py's streams);
  * a call that straddles lo32(n) = 2^32, and one that starts above it;
  * two calls enqueued back to back without a synchronise between them: the table's memory is reused in stream order."""
import os
import re

import numpy as np
import pytest

from helpers import pack_layout, synth

TILE = 576                               # outputs per wave-tile at M = 32
MB = 4                                   # stream bytes per output and channel at M = 32
BLOCK = 256                              # planar blocks of a quarter tile's bytes: every whole block of a call lies in the fixed-order loop's range
BASE = dict(dsd_rate=1, output_rate=88200, channels=2, fmt="P", endianness="L", block_size=BLOCK, filter="E", seed=57)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_binding_states_the_engines_threshold():
    """DITHER_TABLE_MIN_FILES (what the cases below size their batches with) is the engine's kDitherTableMinFiles, and the flag is the header's"""
    import dsd2dxd_amd as d
    src = open(os.path.join(ROOT, "dsd2dxd_amd", "csrc", "d2d_engine.cpp")).read()
    assert "kDitherTableMinFiles = D2D_DITHER_TABLE_MIN_FILES;" in src
    assert int(re.search(r"#define D2D_DITHER_TABLE_MIN_FILES (\d+)", src).group(1)) == d.DITHER_TABLE_MIN_FILES >= 2
    hdr = open(os.path.join(ROOT, "include", "dsd2dxd_amd.h")).read()
    assert int(re.search(r"D2D_DBG_NO_DITHER_TABLE = 1u << (\d+)", hdr).group(1)) == 17 and d.DBG_NO_DITHER_TABLE == 1 << 17


def _chans(nbytes, seed, msb_first=False, dsd_rate=1):
    """a loud sine and pink noise with an all-ones and an all-zeros stretch: both rails at 0 dB, so tiles of the loop take the careful path"""
    x = [synth("sine", nbytes, seed=seed, amp=0.5, freq=900.0, msb_first=msb_first, dsd_rate=dsd_rate).copy(),
         synth("pink", nbytes, seed=seed + 1, amp=0.098, msb_first=msb_first, dsd_rate=dsd_rate).copy()]
    if nbytes >= 3 * TILE * MB:
        x[0][TILE * MB + 40:TILE * MB + 700] = 0xFF
        x[1][2 * TILE * MB - 300:2 * TILE * MB + 500] = 0x00
    return x


def _calls(chans, cuts, kw):
    return [pack_layout([c[a:b] for c in chans], kw["fmt"], kw["block_size"]) for a, b in zip(cuts[:-1], cuts[1:])]


def _oracle(O, kw, calls, seek=0):
    o = O.Oracle(**kw)
    if seek:
        o.seek(seek)
    out = []
    for b in calls:
        if b.size == 0:
            out.append(np.zeros(0, np.uint8))
            continue
        w, fr = o.translate(b)
        out.append(w[:fr * o.frame_bytes].copy())
    peaks = [o.peak(c) for c in range(kw["channels"])]
    o.close()
    return out, peaks


def _engine(d, kw, calls, debug=0, seeks=None, sync_each=True):
    """calls[f][i]: the bytes file f feeds in call i (possibly none).  Returns the frames of every file and call, every file's peaks, whether each
    call used the table, and the kernels' names.  sync_each = False: every call is enqueued before the first synchronise."""
    import torch
    n_files, ncalls, C = len(calls), len(calls[0]), kw["channels"]
    e = d.Engine(n_files=n_files, kernel=2, debug=debug, **kw)
    for f, pos in (seeks or {}).items():
        e.seek(pos, file=f)
    fb = e.frame_bytes
    stream = torch.cuda.current_stream().cuda_stream
    held, used, names = [], [], []
    for i in range(ncalls):
        ios = (d.FileIO * n_files)()
        d_in, d_out = [], []
        for f in range(n_files):
            b = calls[f][i]
            bpc = b.size // C
            nfr = e.next_frames(bpc, file=f)
            d_in.append(torch.from_numpy(b).cuda() if b.size else None)
            d_out.append(torch.zeros((nfr * fb + 31) // 16 * 16, dtype=torch.uint8, device="cuda"))
            ios[f].dsd = d_in[f].data_ptr() if b.size else 0
            ios[f].bytes_per_channel = bpc
            ios[f].pcm = d_out[f].data_ptr(); ios[f].pcm_capacity_bytes = d_out[f].numel()
        before = e.dither_table_calls()
        e.translate_batch_device(ios, stream)
        used.append(e.dither_table_calls() - before)
        names.append(e.kernel_name())
        held.append((ios, d_in, d_out))
        if sync_each:
            torch.cuda.synchronize()
    torch.cuda.synchronize()
    out = [[held[i][2][f][:held[i][0][f].frames_out * fb].cpu().numpy() for i in range(ncalls)] for f in range(n_files)]
    peaks = [[e.peak(c, file=f) for c in range(C)] for f in range(n_files)]
    assert all(u in (0, 1) for u in used)
    e.close()
    return out, peaks, [bool(u) for u in used], names


def _check(d, O, kw, distinct, n_files, expect, kernel, seeks=None, sync_each=True, want=None):
    """distinct: K files as lists of their calls' bytes; file f of the batch is distinct[f % K].  expect: per call, whether the table serves it.
    want: the oracle's (frames of every call, peaks) of the K files where a case has them already."""
    K = len(distinct)
    calls = [distinct[f % K] for f in range(n_files)]
    if want is None:
        want = [_oracle(O, kw, distinct[k], (seeks or {}).get(k, 0)) for k in range(K)]
    on = _engine(d, kw, calls, 0, seeks, sync_each)
    off = _engine(d, kw, calls, d.DBG_NO_DITHER_TABLE, seeks, sync_each)
    assert off[2] == [False] * len(expect), off[2]
    assert on[2] == list(expect), (on[2], expect)
    assert on[3] == off[3] == [kernel] * len(expect), (on[3], off[3])       # one name for both forms of the kernel
    for f in range(n_files):
        w_out, w_peaks = want[f % K]
        for i in range(len(expect)):
            for tag, got in (("table", on[0][f][i]), ("hashed", off[0][f][i])):
                if not np.array_equal(got, w_out[i]):
                    k = int(np.flatnonzero(got != w_out[i])[0]) if got.size == w_out[i].size else -1
                    raise AssertionError(f"{tag}: file {f}, call {i}: {got.size} bytes against the oracle's {w_out[i].size}, first differing byte {k}; {on[3][i]}")
        assert on[1][f] == off[1][f] == w_peaks, (f, on[1][f], off[1][f], w_peaks)
    return on


# ---- call lengths around a tile ----
# outputs of each call: shorter than a tile; one tile; one tile + 1; 3 tiles + 5 in two ragged calls (the second starts inside a tile and a block)
LENGTHS = {"short": [TILE - 123], "one_tile": [TILE], "one_tile_plus_1": [TILE + 1], "three_tiles_plus_5_ragged": [TILE + 211, 2 * TILE - 206]}
K24T = "d2d_fir_mx_kernel<4, 560, 3, 1, 3, 1, 5>"


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(LENGTHS))
def test_lengths_around_a_tile(engine_lib, oracle_mod, case):
    d = engine_lib
    outs = LENGTHS[case]
    assert case != "three_tiles_plus_5_ragged" or sum(outs) == 3 * TILE + 5
    cuts = [0] + [MB * int(n) for n in np.cumsum(outs)]
    kw = dict(BASE, bit_depth=24, dither="T")
    distinct = [_calls(_chans(cuts[-1], 11 + 2 * k), cuts, kw) for k in range(2)]
    _check(d, oracle_mod, kw, distinct, d.DITHER_TABLE_MIN_FILES, [True] * len(outs), K24T)


# ---- every instantiation that reads the table, and the dithered formats that do not ----
# (bits, dither, level) -> the kernel's (KIND, SBY); KIND 1, 2 (the integer requantiser) read the table
FORMATS = {"s24_T": (24, "T", 0.0, (1, 3)), "s24_R": (24, "R", 0.0, (2, 3)), "s16_T": (16, "T", 0.0, (1, 2)), "s16_R": (16, "R", 0.0, (2, 2)),
           "s20_T": (20, "T", 0.0, (5, 3)), "s24_T_minus3dB": (24, "T", -3.0, (5, 3)), "s24_R_minus3dB": (24, "R", -3.0, (6, 3)),
           "s16_T_minus3dB": (16, "T", -3.0, (5, 2)), "s16_R_minus3dB": (16, "R", -3.0, (6, 2)), "f32_F": (32, "F", 0.0, (7, 4))}
NOUT = 5 * TILE + 5                      # three calls: whole blocks (its second tile runs the loop), a ragged middle, the tail
CUTS = [0, BLOCK * 20, BLOCK * 33 + 77, MB * NOUT]


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", sorted(FORMATS))
def test_formats(engine_lib, oracle_mod, fmt):
    d = engine_lib
    bits, dither, level, (kind, sby) = FORMATS[fmt]
    kw = dict(BASE, bit_depth=bits, dither=dither, level_db=level)
    distinct = [_calls(_chans(CUTS[-1], 21 + 2 * k), CUTS, kw) for k in range(2)]
    _check(d, oracle_mod, kw, distinct, d.DITHER_TABLE_MIN_FILES, [kind in (1, 2)] * 3, "d2d_fir_mx_kernel<4, 560, 3, %d, %d, 1, 5>" % (kind, sby))


@pytest.mark.gpu
@pytest.mark.parametrize("dsd_rate,out_rate,filt,taps,bits,dither,ks", [(1, 88200, "X", 384, 16, "R", (2, 2)), (2, 176400, "C", 512, 24, "T", (1, 3))],
                         ids=["X_M32_s16_R", "C_M32_s24_T"])
def test_the_other_m32_filters(engine_lib, oracle_mod, dsd_rate, out_rate, filt, taps, bits, dither, ks):
    d = engine_lib
    kw = dict(BASE, dsd_rate=dsd_rate, output_rate=out_rate, filter=filt, bit_depth=bits, dither=dither)
    distinct = [_calls(_chans(CUTS[-1], 71 + 2 * k, dsd_rate=dsd_rate), CUTS, kw) for k in range(2)]
    _check(d, oracle_mod, kw, distinct, d.DITHER_TABLE_MIN_FILES, [True] * 3, "d2d_fir_mx_kernel<4, %d, 3, %d, %d, 1, 5>" % ((taps,) + ks))


@pytest.mark.gpu
def test_byte_interleaved_stereo(engine_lib, oracle_mod):
    d = engine_lib
    kw = dict(BASE, fmt="I", endianness="M", block_size=1, bit_depth=24, dither="T")
    cuts = [0, BLOCK * 20 + 7, BLOCK * 33 + 1, MB * NOUT]
    distinct = [_calls(_chans(cuts[-1], 31 + 2 * k, msb_first=True), cuts, kw) for k in range(2)]
    _check(d, oracle_mod, kw, distinct, d.DITHER_TABLE_MIN_FILES, [True] * 3, K24T)


@pytest.mark.gpu
def test_every_wave_walks_several_tiles(engine_lib, oracle_mod):
    """128 files of 40.4 tiles: two blocks of eight waves per file, so a wave takes two or three tiles through both regions of the loop and its drain
    with the words of the next region in flight; the second call's table starts at index 20 736 + 1"""
    d = engine_lib
    kw = dict(BASE, block_size=4096, bit_depth=24, dither="T")
    nbytes = MB * (40 * TILE + 233)
    cuts = [0, MB * (36 * TILE + 1), nbytes]
    distinct = []
    for k in range(2):
        ch = _chans(nbytes, 41 + 2 * k)
        ch[k][MB * 9 * TILE + 100:MB * 9 * TILE + 1500] = 0xFF          # a clipped stretch further in: careful tiles between tiles that read the table
        distinct.append(_calls(ch, cuts, kw))
    _check(d, oracle_mod, kw, distinct, 128, [True, True], K24T)


# ---- files of different length ----
@pytest.mark.gpu
def test_ragged_batch_one_file_ends_in_the_first_call(engine_lib, oracle_mod):
    """a threshold's worth of files and one more that ends in the first call: every call's files that still produce outputs start at one index,
    so every call reads the table, whose length is the longest file's"""
    d = engine_lib
    n = d.DITHER_TABLE_MIN_FILES + 1
    kw = dict(BASE, bit_depth=24, dither="T")
    c1 = BLOCK * 24                                                      # first call: 1536 outputs
    ends = [MB * (5 * TILE + 5 - 17 * f) for f in range(n - 1)] + [BLOCK * 11 + 36]      # the last file: 713 outputs, all in the first call
    distinct = []
    for f in range(n):
        ch = _chans(ends[f], 81 + 2 * f)
        cuts = [0, min(c1, ends[f]), max(c1, ends[f])] if f < n - 1 else [0, ends[f], ends[f]]
        distinct.append(_calls(ch, cuts, kw))
    assert distinct[-1][1].size == 0
    _check(d, oracle_mod, kw, distinct, n, [True, True], K24T)


# ---- calls the table does not serve ----
@pytest.mark.gpu
def test_a_file_moved_ahead_keeps_the_batch_off_the_table(engine_lib, oracle_mod):
    """d2d_seek puts one file at another index: its words are not the others', and every file of every call hashes its own"""
    d = engine_lib
    n = d.DITHER_TABLE_MIN_FILES + 1
    kw = dict(BASE, bit_depth=24, dither="T")
    distinct = [_calls(_chans(CUTS[-1], 91 + 2 * f), CUTS, kw) for f in range(n)]
    _check(d, oracle_mod, kw, distinct, n, [False] * 3, K24T, seeks={1: MB * 1000})


@pytest.mark.gpu
def test_one_file_fewer_than_the_threshold(engine_lib, oracle_mod):
    d = engine_lib
    kw = dict(BASE, bit_depth=24, dither="T")
    n = d.DITHER_TABLE_MIN_FILES - 1
    distinct = [_calls(_chans(CUTS[-1], 101 + 2 * f), CUTS, kw) for f in range(n)]
    _check(d, oracle_mod, kw, distinct, n, [False] * 3, K24T)


# ---- the careful path next to tiles that read the table ----
@pytest.mark.gpu
def test_exact_ties_take_the_careful_path(engine_lib, oracle_mod):
    """the input of tests/test_gpu_mx_resident.py that holds exact negative ties and both rails: the tiles redone from the burst's integers hash their
    words (noise()) while their neighbours read them from the table"""
    from test_gpu_mx_resident import CUTS as RCUTS, KW_CAREFUL, _calls as rcalls, _careful_files, _careful_oracle
    want, _ = _careful_oracle(oracle_mod)
    distinct = [rcalls(ch, "P", RCUTS) for ch in _careful_files()]
    K = len(distinct)
    n_files = K * -(-engine_lib.DITHER_TABLE_MIN_FILES // K)             # every file and as many twins as the threshold asks for
    _check(engine_lib, oracle_mod, KW_CAREFUL, distinct, n_files, [True] * 3, K24T, want=want)


@pytest.mark.gpu
@pytest.mark.parametrize("bits,dither,ks", [(24, "T", (1, 3)), (16, "R", (2, 2))], ids=["t24", "r16"])
def test_both_rails_on_the_adversarial_streams(engine_lib, oracle_mod, bits, dither, ks):
    """every window follows the sign of the taps or of a digit: outputs beyond full scale in both polarities at every index modulo the tile"""
    from helpers import decode_pcm
    from test_gpu_extreme_sums import _stream
    d = engine_lib
    streams = [_stream(1, 88200, "E", 24, None, 500 + c, (c, 2), False) for c in range(2)]
    chans = [st.packed(False) for st in streams]
    n = chans[0].size
    kw = dict(BASE, block_size=4096, seed=21, bit_depth=bits, dither=dither)
    a = 4096 * max(1, n // 4096 // 3)
    cuts = [0, a, 2 * a + 333, n]
    on = _check(d, oracle_mod, kw, [_calls(chans, cuts, kw)], d.DITHER_TABLE_MIN_FILES, [True] * 3, "d2d_fir_mx_kernel<4, 560, 3, %d, %d, 1, 5>" % ks)
    pcm = decode_pcm(np.concatenate(on[0][0]), bits, 2)
    lim = 1 << (bits - 1)
    assert all(pcm[:, c].max() == lim - 1 and pcm[:, c].min() == -lim for c in range(2))


# ---- the index wrap ----
@pytest.mark.gpu
@pytest.mark.parametrize("bits,dither,level,ks", [(24, "T", 0.0, (1, 3)), (16, "R", 0.0, (2, 2))], ids=["s24_T", "s16_R"])
def test_a_call_straddles_index_2_pow_32(engine_lib, oracle_mod, bits, dither, level, ks):
    """every file is put 2 tiles + 300 outputs below index 2^32 (d2d_seek, orc_seek); the first call's table holds words of both sides of the wrap
    (the tile that holds the wrap takes the careful path, the tiles behind it read words made with the key stepped once more), the second call
    starts above it with hi32 folded into the key"""
    d = engine_lib
    kw = dict(BASE, block_size=4096, bit_depth=bits, dither=dither, level_db=level)
    n0 = (1 << 32) - (2 * TILE + 300)
    outs = [16 * TILE + 17, 8 * TILE + 5]
    cuts = [0] + [MB * int(n) for n in np.cumsum(outs)]
    n = d.DITHER_TABLE_MIN_FILES
    distinct = [_calls(_chans(cuts[-1], 111 + 2 * k), cuts, kw) for k in range(2)]
    _check(d, oracle_mod, kw, distinct, n, [True, True], "d2d_fir_mx_kernel<4, 560, 3, %d, %d, 1, 5>" % ks, seeks={f: MB * n0 for f in range(n)})


# ---- the table's memory from call to call ----
@pytest.mark.gpu
def test_two_calls_back_to_back_without_a_synchronise(engine_lib, oracle_mod):
    """the second call's fill is enqueued while the first call's kernel may still read the table: the stream orders them.  (The second call is
    the shorter one, so the table does not grow and nothing synchronises inside the engine either.)"""
    d = engine_lib
    kw = dict(BASE, block_size=4096, bit_depth=24, dither="T")
    cuts = [0, 4096 * 22, 4096 * 22 + MB * (9 * TILE + 77)]
    distinct = [_calls(_chans(cuts[-1], 121 + 2 * k), cuts, kw) for k in range(2)]
    _check(d, oracle_mod, kw, distinct, 2 * d.DITHER_TABLE_MIN_FILES, [True, True], K24T, sync_each=False)
