"""The fp6 kernel's resident flavours (M = 32, stereo frames) expand a chain's B operands a step or two ahead, step 0's inside the burst
(D2D_MX_FEED).  The same cases also ran a build that carried the base-32 digit weights in the A scales of the matrix rows and
recombined by additions (measured no faster and not in the tree: profiles/rowscale_check.md); they are kept for what they reach.  Bit-equality
with the oracle at the smallest shapes that reach every path of the chain and of the recombination:
  * the burst of the fixed-order loop (inner tiles of a call), its drain, the careful path from the burst's integers (redo_v) and the tiles at a
    call's edges, whose chain is run again and recombined sample by sample (recombine): calls shorter than a tile, of exactly one tile, one
    tile + 1 output, and 3 tiles + 5 outputs in two ragged calls;
  * the three dither kinds at 24 bits, 16 bits, float frames (their accumulators start from a value in the digit-4 rows), the f64 flavour;
  * byte-interleaved stereo, a mono stream as a planar pair, two files of different length in one batch;
  * the adversarial streams of tests/adversarial.py, which attain the extremes of every digit sum and f32 part, on the production routes of the four
    M = 32 tables (A_M32 runs the scratch flavour, whose chain is unchanged: its neighbours' objects changed);
  * the input of tests/test_gpu_mx_resident.py that holds exact negative ties."""
import numpy as np
import pytest

import adversarial as A
from helpers import pack_layout, synth
from test_gpu_extreme_sums import KERNELS_A, _conversion, _format_kw, _stream, convert
from test_gpu_mx_resident import KW_CAREFUL, _careful_files, _careful_oracle, _run_tiled, _targs

pytestmark = pytest.mark.gpu

TILE = 576                               # outputs per wave-tile at M = 32
MB = 4                                   # stream bytes per output and channel (DSD64 -> 88.2 kHz)
BLOCK = 256                              # planar blocks of a quarter tile's bytes: every whole block of a call lies in the fixed-order loop's range
BASE = dict(dsd_rate=1, output_rate=88200, channels=2, fmt="P", endianness="L", block_size=BLOCK, filter="E", seed=57)


def _chans(nbytes, seed, msb_first=False):
    """a loud sine and pink noise with an all-ones and an all-zeros stretch: both rails at 0 dB, so tiles of the loop take the careful path"""
    x = [synth("sine", nbytes, seed=seed, amp=0.5, freq=900.0, msb_first=msb_first).copy(), synth("pink", nbytes, seed=seed + 1, amp=0.098, msb_first=msb_first).copy()]
    if nbytes >= 3 * TILE * MB:
        x[0][TILE * MB + 40:TILE * MB + 700] = 0xFF
        x[1][2 * TILE * MB - 300:2 * TILE * MB + 500] = 0x00
    return x


def _run(engine_lib, oracle_mod, kw, chans, cuts):
    """one engine and one oracle over the calls chans[:, a:b]: equal frames, bytes and peaks; returns the kernels' names"""
    e = engine_lib.Engine(kernel=2, **kw)
    o = oracle_mod.Oracle(**kw)
    names = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        buf = pack_layout([c[a:b] for c in chans], kw["fmt"], kw["block_size"])
        g, gf = e.translate(buf)
        w, wf = o.translate(buf)
        assert gf == wf, (a, b, gf, wf)
        w = w[:wf * o.frame_bytes]
        if not np.array_equal(g, w):
            first = int(np.flatnonzero(g != w)[0]) // o.frame_bytes
            raise AssertionError(f"call [{a}, {b}): first differing frame {first} of {wf} (index mod tile {first % TILE}); {int((g != w).sum())} bytes differ; {e.kernel_name()}")
        names.append(e.kernel_name())
    C_ = kw["channels"]
    assert [e.peak(c) for c in range(C_)] == [o.peak(c) for c in range(C_)]
    e.close()
    o.close()
    print("kernels:", names)
    return names


# outputs of each call: shorter than a tile; one tile; one tile + 1; 3 tiles + 5 in two ragged calls (the second starts inside a tile and a block)
LENGTHS = {"short": [TILE - 123], "one_tile": [TILE], "one_tile_plus_1": [TILE + 1], "three_tiles_plus_5_ragged": [TILE + 211, 2 * TILE - 206]}


@pytest.mark.parametrize("case", sorted(LENGTHS))
def test_lengths_around_a_tile(engine_lib, oracle_mod, case):
    outs = LENGTHS[case]
    assert case != "three_tiles_plus_5_ragged" or sum(outs) == 3 * TILE + 5
    cuts = [0] + [MB * n for n in np.cumsum(outs)]
    kw = dict(BASE, bit_depth=24, dither="T")
    names = _run(engine_lib, oracle_mod, kw, _chans(cuts[-1], 11), cuts)
    assert all(n == "d2d_fir_mx_kernel<4, 560, 3, 1, 3, 1, 5>" for n in names), names


FORMATS = {"s24_T": (24, "T", 0.0, (1, 3)), "s24_R": (24, "R", 0.0, (2, 3)), "s24_X": (24, "X", 0.0, (0, 3)), "s16_T": (16, "T", 0.0, (1, 2)),
           "f32_X": (32, "X", 0.0, (0, 4)), "s24_T_minus3dB": (24, "T", -3.0, (5, 3))}
NOUT = 5 * TILE + 5                      # three calls: whole blocks, a ragged middle, the tail
CUTS = [0, BLOCK * 20, BLOCK * 33 + 77, MB * NOUT]


@pytest.mark.parametrize("fmt", sorted(FORMATS))
def test_formats(engine_lib, oracle_mod, fmt):
    bits, dither, level, (kind, sby) = FORMATS[fmt]
    kw = dict(BASE, bit_depth=bits, dither=dither, level_db=level)
    names = _run(engine_lib, oracle_mod, kw, _chans(CUTS[-1], 21), CUTS)
    assert all(n == "d2d_fir_mx_kernel<4, 560, 3, %d, %d, 1, 5>" % (kind, sby) for n in names), names


def test_byte_interleaved_stereo(engine_lib, oracle_mod):
    kw = dict(BASE, fmt="I", endianness="M", block_size=1, bit_depth=24, dither="T")
    names = _run(engine_lib, oracle_mod, kw, _chans(CUTS[-1], 31, msb_first=True), [0, BLOCK * 20 + 7, BLOCK * 33 + 1, MB * NOUT])
    assert all(n == "d2d_fir_mx_kernel<4, 560, 3, 1, 3, 1, 5>" for n in names), names


def test_mono_stream_as_a_planar_pair(engine_lib, oracle_mod):
    """a call of two equal halves of whole blocks runs the halves side by side as the channels of a pair (3 072 outputs = 5.3 tiles each)"""
    half = 4096 * 3
    x = synth("sine", 2 * half + 1300, seed=41, amp=0.5).copy()
    x[3000:3700] = 0xFF; x[half + 5000:half + 5600] = 0x00
    kw = dict(BASE, channels=1, block_size=4096, bit_depth=24, dither="T")
    names = _run(engine_lib, oracle_mod, kw, [x], [0, 2 * half, x.size])
    assert names[0].startswith("d2d_fir_mx_kernel<4, 560, 3, 1, 3"), names


def test_two_files_of_different_length_in_one_batch(engine_lib, oracle_mod):
    import torch
    kw = dict(BASE, bit_depth=24, dither="T")
    lens = [MB * (4 * TILE + 5), MB * (2 * TILE - 77)]
    files = [_chans(n, 51 + 2 * f) for f, n in enumerate(lens)]
    e = engine_lib.Engine(n_files=2, kernel=2, **kw)
    fb = e.frame_bytes
    d_in = [torch.from_numpy(pack_layout(ch, "P", BLOCK)).cuda() for ch in files]
    nfr = [e.next_frames(n, file=f) for f, n in enumerate(lens)]
    d_out = [torch.zeros((n * fb + 31) // 16 * 16, dtype=torch.uint8, device="cuda") for n in nfr]
    ios = (engine_lib.FileIO * 2)()
    for f in range(2):
        ios[f].dsd = d_in[f].data_ptr(); ios[f].bytes_per_channel = lens[f]
        ios[f].pcm = d_out[f].data_ptr(); ios[f].pcm_capacity_bytes = d_out[f].numel()
    e.translate_batch_device(ios, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert e.kernel_name() == "d2d_fir_mx_kernel<4, 560, 3, 1, 3, 1, 5>"
    for f in range(2):
        o = oracle_mod.Oracle(**kw)
        w, wf = o.translate(pack_layout(files[f], "P", BLOCK))
        assert ios[f].frames_out == wf == nfr[f]
        assert np.array_equal(d_out[f][:wf * fb].cpu().numpy(), w[:wf * fb]), f
        assert [e.peak(c, file=f) for c in range(2)] == [o.peak(c) for c in range(2)]
        o.close()
    e.close()


@pytest.mark.parametrize("fam,name,fmt", [("fir", n, x) for n in ("E_M32", "X_M32", "C_M32") for x in ("f32", "t24", "r16", "t24_level")] + [("cascade", "A_M32", "t24")])
def test_extreme_sums_on_the_production_route(engine_lib, oracle_mod, fam, name, fmt):
    """every part at its attainable extreme, in both polarities, at every output index modulo the tile (tests/test_gpu_extreme_sums.py's
    builder and comparison; float frames are also compared with the closed form)"""
    assert A.tables()["filters"][name]["M"] == 32
    dsd_rate, out_rate, filt = _conversion(fam, name)
    streams = [_stream(dsd_rate, out_rate, filt, 24, None, 500 + c, (c, 2), False) for c in range(2)]
    kw = dict(dsd_rate=dsd_rate, output_rate=out_rate, channels=2, fmt="P", endianness="L", block_size=4096, filter=filt, seed=21, **_format_kw(fmt, streams[0]))
    got = convert(engine_lib, oracle_mod, kw, streams, KERNELS_A[name, fmt], closed_form=fmt == "f32" and fam == "fir", rails=fmt in ("t24", "r16") and fam == "fir")
    assert got.size


def test_careful_path_on_exact_negative_ties(engine_lib, oracle_mod):
    """tiles that clip or hold an exact tie are redone from the integers the burst took: the burst's v feeds the careful path"""
    want, _ = _careful_oracle(oracle_mod)
    e, got = _run_tiled(engine_lib, oracle_mod, KW_CAREFUL, _careful_files(), want=want)
    assert _targs(e)[:5] == ["4", "560", "3", "1", "3"], e.kernel_name()
    assert all(g.size for g in got)
