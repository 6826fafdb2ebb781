"""The fp6 kernel's stereo frame flavours at M = 32 (d2d_fir_mx_kernel<4, ...>) keep their tap fragments in registers and take a draining
accumulator set's integers in one burst at the start of a region.  Bit-equality with the oracle on shapes where every wave
of a block walks several tiles through both regions of the fixed-order loop and its drain: a batch of 256 files of about 30 tiles each (one
block per file), two (or a few) distinct files among them compared with the oracle and every other file with its twin."""
import numpy as np
import pytest

from helpers import decode_pcm, pack_layout, synth

TILE = 576                               # outputs per wave-tile at M = 32: 32 columns x 3 groups x 6 phases
N_FILES = 256
BLOCK = 4096
NBYTES = BLOCK * 17 + 300                # per channel at DSD64 -> 88.2 kHz (4 bytes per output): 17 483 outputs = 30.4 tiles
# the first call holds 24.9 tiles (each of a block's eight waves walks at least three); then 3.6 tiles; the last is 1099 outputs: no whole number of tiles
CUTS = [0, BLOCK * 14, BLOCK * 16, NBYTES]


def _calls(chans, fmt, cuts):
    return [pack_layout([ch[a:b] for ch in chans], fmt, BLOCK if fmt == "P" else 1) for a, b in zip(cuts[:-1], cuts[1:])]


def _oracle_run(oracle_mod, kw, calls):
    o = oracle_mod.Oracle(**kw)
    out = []
    for b in calls:
        w, fr = o.translate(b)
        out.append(w[:fr * o.frame_bytes].copy())
    return out, [o.peak(c) for c in range(kw["channels"])]


def _run_tiled(engine_lib, oracle_mod, kw, distinct, fmt="P", cuts=CUTS, want=None):
    """distinct: K files (lists of channels); file f of the batch is distinct[f % K].  Every call of the K first files equals the oracle's
    bytes, every other file its twin's; peaks alike.  Returns the engine and the K files' bytes.  want: oracle results computed before."""
    import torch
    K, C_ = len(distinct), kw["channels"]
    e = engine_lib.Engine(n_files=N_FILES, kernel=2, **kw)
    fb = e.frame_bytes
    calls = [_calls(ch, fmt, cuts) for ch in distinct]
    if want is None:
        want = [_oracle_run(oracle_mod, kw, calls[k]) for k in range(K)]
    got = [[] for _ in range(K)]
    stream = torch.cuda.current_stream().cuda_stream
    for i in range(len(cuts) - 1):
        bpc = calls[0][i].size // C_
        d_in = [torch.from_numpy(calls[k][i]).cuda() for k in range(K)]          # twins read the same device bytes
        nfr = e.next_frames(bpc, file=0)
        cap = (nfr * fb + 31) // 16 * 16                                          # (a file's frames start at a 16-byte boundary)
        d_out = torch.zeros(N_FILES, cap, dtype=torch.uint8, device="cuda")
        ios = (engine_lib.FileIO * N_FILES)()
        for f in range(N_FILES):
            assert e.next_frames(bpc, file=f) == nfr
            ios[f].dsd = d_in[f % K].data_ptr(); ios[f].bytes_per_channel = bpc
            ios[f].pcm = d_out[f].data_ptr(); ios[f].pcm_capacity_bytes = cap
        e.translate_batch_device(ios, stream)
        torch.cuda.synchronize()
        assert all(ios[f].frames_out == nfr for f in range(N_FILES))
        for k in range(K):
            g = d_out[k, :nfr * fb].cpu().numpy()
            assert np.array_equal(g, want[k][0][i]), (k, i, e.kernel_name())
            got[k].append(g)
            twins = d_out[k::K]
            assert bool((twins == twins[0:1]).all()), (k, i)
    for f in range(N_FILES):
        assert [e.peak(c, file=f) for c in range(C_)] == want[f % K][1], f
    return e, [np.concatenate(g) for g in got]


def _targs(e):
    return [t.strip() for t in e.kernel_name().split("<")[1].rstrip(">").split(",")]


def _two_files(dsd_rate=1, msb_first=False, nbytes=NBYTES):
    return [[synth("sine" if (c + f) % 2 else "pink", nbytes, seed=300 + 10 * f + c, dsd_rate=dsd_rate, msb_first=msb_first,
                   freq=700.0 * (f + 1), amp=0.45 if (c + f) % 2 else 0.098) for c in range(2)] for f in range(2)]


@pytest.mark.gpu
@pytest.mark.parametrize("bits,dither,level", [(24, "T", 0.0), (24, "R", 0.0), (16, "T", 0.0), (24, "X", 0.0), (32, "X", 0.0), (24, "T", -3.0)],
                         ids=["s24_T", "s24_R", "s16_T", "s24_none", "f32_none", "s24_T_minus3dB"])
def test_stereo_dsd64_to_88k2_every_wave_walks_several_tiles(engine_lib, oracle_mod, bits, dither, level):
    """Stereo DSD64 -> 88.2 kHz, E filter: the integer requantiser's three dither kinds and two depths, float frames, and the f64
    requantiser (-3 dB), over ragged calls and a last call that is no whole number of tiles."""
    kw = dict(dsd_rate=1, output_rate=88200, channels=2, fmt="P", endianness="L", block_size=BLOCK, filter="E",
              bit_depth=bits, dither=dither, seed=41, level_db=level)
    e, _ = _run_tiled(engine_lib, oracle_mod, kw, _two_files())
    t = _targs(e)
    assert e.kernel_name().startswith("d2d_fir_mx_kernel") and t[:3] == ["4", "560", "3"] and t[4] == str(bits // 8), e.kernel_name()
    assert (int(t[3]) >= 4) == (level != 0.0), e.kernel_name()


# ---- the careful path inside the pipelined loop ----
N_CAREFUL = 18                           # distinct files: 18 x 17 483 = 314 694 outputs per channel under triangular dither
KW_CAREFUL = dict(dsd_rate=1, output_rate=88200, channels=2, fmt="P", endianness="L", block_size=BLOCK, filter="E",
                  bit_depth=24, dither="T", seed=99, level_db=0.0)
_careful = {}


def _careful_files():
    """sines with all-ones / all-zeros stretches of 200-3000 bytes inside the first call's inner tiles (tiles 3 .. 21 of 24.9: both rails)"""
    if "files" not in _careful:
        rng = np.random.default_rng(7)
        files = []
        for f in range(N_CAREFUL):
            chans = []
            for c in range(2):
                x = synth("sine", NBYTES, seed=500 + 2 * f + c, freq=300.0 + 170.0 * f + 40.0 * c, amp=0.4).copy()
                for k in range(3):
                    n = int(rng.integers(200, 3001))
                    a = int(rng.integers(3 * TILE * 4, 21 * TILE * 4 - n))
                    x[a:a + n] = 0xFF if (f + c + k) % 2 else 0x00
                chans.append(x)
            files.append(chans)
        _careful["files"] = files
    return _careful["files"]


def _careful_oracle(oracle_mod):
    """the oracle's bytes and peaks of every call (computed once), and its f64 samples y of the whole files"""
    if "want" not in _careful:
        files = _careful_files()
        _careful["want"] = [_oracle_run(oracle_mod, KW_CAREFUL, _calls(ch, "P", CUTS)) for ch in files]
        ys = []
        for ch in files:
            o = oracle_mod.Oracle(**KW_CAREFUL)
            _, fr, y = o.translate(pack_layout(ch, "P", BLOCK), want_f64=True)
            ys.append(y[:fr].copy())
        _careful["y"] = ys
    return _careful["want"], _careful["y"]


def test_the_careful_input_holds_exact_ties_that_the_two_roundings_resolve_differently(oracle_mod):
    """On the CPU: q = y 2^23 + d is exact in f64 (y = v 2^-28, d a multiple of 2^-16); among the 2 x 314 694 samples of the input below some
    are exact ties (q - floor(q) = 1/2), and at least one of them is negative: there the fast epilogue's rounding (half up, floor(q + 1/2))
    and the definition's (half away from zero) differ, so only a tile redone the careful way gives the oracle's sample."""
    _, ys = _careful_oracle(oracle_mod)
    ties = differ = 0
    seed = KW_CAREFUL["seed"]
    nmax = max(y.shape[0] for y in ys)
    words = [np.array([oracle_mod.rng(seed, c, i) for i in range(nmax)], dtype=np.int64) for c in range(2)]
    for y in ys:
        for c in range(2):
            w = words[c][:y.shape[0]]
            d = ((w & 0xFFFF) + (w >> 16) + 1).astype(np.float64) * 2.0 ** -16 - 1.0
            q = y[:, c] * 2.0 ** 23 + d
            tie = (q - np.floor(q)) == 0.5
            inside = np.abs(q) < 2.0 ** 23 - 2
            ties += int((tie & inside).sum())
            differ += int((tie & inside & (q < 0)).sum())
    assert sum(y.shape[0] for y in ys) >= 300_000
    print("exact ties:", ties, "of them negative:", differ)
    assert ties >= 1 and differ >= 1, (ties, differ)


@pytest.mark.gpu
def test_careful_tiles_inside_the_pipelined_loop(engine_lib, oracle_mod):
    """Tiles that clip or hold an exact tie are redone sample by sample from the integers the burst took (the accumulators they came from
    are overwritten by then): both rails are reached, bytes and peaks are the oracle's."""
    want, _ = _careful_oracle(oracle_mod)
    e, got = _run_tiled(engine_lib, oracle_mod, KW_CAREFUL, _careful_files(), want=want)
    assert _targs(e)[:5] == ["4", "560", "3", "1", "3"], e.kernel_name()
    pcm = np.concatenate([decode_pcm(g, 24, 2) for g in got])
    assert pcm.max() == (1 << 23) - 1 and pcm.min() == -(1 << 23)


# ---- the other M = 32 rows, a mono stream as a planar pair, byte-interleaved stereo ----
@pytest.mark.gpu
@pytest.mark.parametrize("dsd_rate,out_rate,filt,taps", [(1, 88200, "X", "384"), (2, 176400, "C", "512")], ids=["X_M32", "C_M32"])
def test_the_other_stereo_m32_filters(engine_lib, oracle_mod, dsd_rate, out_rate, filt, taps):
    kw = dict(dsd_rate=dsd_rate, output_rate=out_rate, channels=2, fmt="P", endianness="L", block_size=BLOCK, filter=filt,
              bit_depth=24, dither="T", seed=43, level_db=0.0)
    e, _ = _run_tiled(engine_lib, oracle_mod, kw, _two_files(dsd_rate), cuts=CUTS)
    assert e.kernel_name().startswith("d2d_fir_mx_kernel") and _targs(e)[:5] == ["4", taps, "3", "1", "3"], e.kernel_name()


@pytest.mark.gpu
def test_a_m32_feeds_the_48k_cascade(engine_lib, oracle_mod):
    """A_M32 (DSD256 -> 96 kHz: stage A of the cascade) runs the kernel's scratch flavour, whose fragments stay in LDS: its own case, so that the
    row's object is run next to its resident neighbours."""
    nbytes = BLOCK * 24
    chans = [synth("sine", nbytes, seed=61, dsd_rate=4, amp=0.45), synth("pink", nbytes, seed=62, dsd_rate=4, amp=0.098)]
    kw = dict(dsd_rate=4, output_rate=96000, channels=2, fmt="P", endianness="L", block_size=BLOCK, filter="E", bit_depth=24, dither="T", seed=44)
    e = engine_lib.Engine(kernel=2, **kw)
    o = oracle_mod.Oracle(**kw)
    for a, b in [(0, BLOCK * 20), (BLOCK * 20, nbytes)]:
        buf = pack_layout([ch[a:b] for ch in chans], "P", BLOCK)
        g, gf = e.translate(buf)
        w, wf = o.translate(buf)
        assert gf == wf and np.array_equal(g, w[:wf * e.frame_bytes]), (a, b)
    assert [e.peak(c) for c in range(2)] == [o.peak(c) for c in range(2)]


@pytest.mark.gpu
def test_a_mono_stream_as_a_planar_pair(engine_lib, oracle_mod):
    """each half of a call is 30 tiles: the block's eight waves walk three or four tiles of both halves"""
    half = BLOCK * 17
    x = synth("sine", 2 * half + 4396, seed=71, amp=0.5).copy()
    x[20000:22000] = 0xFF; x[half + 30000:half + 31500] = 0x00
    kw = dict(dsd_rate=1, output_rate=88200, channels=1, fmt="P", endianness="L", block_size=BLOCK, filter="E", bit_depth=24, dither="T", seed=77)
    e = engine_lib.Engine(kernel=2, **kw)
    o = oracle_mod.Oracle(**kw)
    names = []
    for a, b in [(0, 2 * half), (2 * half, x.size)]:
        g, gf = e.translate(x[a:b])
        r, rf = o.translate(x[a:b])
        assert gf == rf and np.array_equal(g, r[:rf * o.frame_bytes]), (a, b, e.kernel_name())
        names.append(e.kernel_name())
    assert names[0].startswith("d2d_fir_mx_kernel<4, 560, 3, 1, 3"), names        # whole blocks: the pair route
    assert e.peak(0) == o.peak(0)


@pytest.mark.gpu
def test_byte_interleaved_stereo_input(engine_lib, oracle_mod):
    """the DFF layout: the wave pulls the channels apart inside its staging and runs the loop's interleaved instance"""
    kw = dict(dsd_rate=1, output_rate=88200, channels=2, fmt="I", endianness="M", block_size=1, filter="E", bit_depth=24, dither="T", seed=45)
    e, _ = _run_tiled(engine_lib, oracle_mod, kw, _two_files(msb_first=True), fmt="I", cuts=[0, BLOCK * 14 + 7, BLOCK * 16 + 1, NBYTES])
    assert e.kernel_name().startswith("d2d_fir_mx_kernel") and _targs(e)[:5] == ["4", "560", "3", "1", "3"], e.kernel_name()
