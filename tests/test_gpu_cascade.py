"""Filter 'S' (D2D_FILTER_EQUIRIPPLE_CASCADE, include/dsd2dxd_amd.h) on the GPU: the two-stage definition of the 48 kHz multiples -- stage A into
the scratch, stage B (polyphase L/147) out of it -- bit for bit the CPU oracle in its cascade mode, on every rate pair that filter 'E' serves with
a composed one-pass table, through every entry point the letter passes.

The call lengths follow stage B's tiling: one stage-A sample is one byte per channel at DSD64 (two at DSD128, four at DSD256), 147 of them are one
L/147 cycle, a tile is eight cycles for stereo (1176 samples).  cascade_cases.RAGGED, scaled by the DSD rate, is a single sample, calls that end
mid-cycle, calls just below, at and just above a tile, and several tiles with a remainder; cascade_cases.PLANAR is three calls of whole blocks.  Under
the oracle's rule (frame n exists once stage A has produced ceil(147 n / L) samples) the very first sample already yields frame 0, so the series
has no call without a frame: DRIP adds one (single samples behind the first).

The expected bytes of the stereo 24-bit cases are tests/golden/cascade_digests.json too (tests/test_cascade_cpu.py holds the oracle to that file), and
the kernel names are tests/golden/route_cascade.json's.  An engine without the letter refuses every create here with D2D_ERR_FILTER."""
import ctypes as C
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

from cascade_cases import (COMPOSED, CONTROL, IL, PL, PLANAR, call_buffers, golden_cases, make_channels, oracle_run, pair_id, ragged_calls,
                           recipe_for)
from helpers import pack_layout, random_bytes, synth, write_dsf

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CLI = os.path.join(ROOT, "dsd2dxd_amd", "dsd2dxd_amd_cli")
AUTO, LUT, MFMA = 0, 1, 2
GUARD = 4096
DRIP = (1, 1, 1, 1, 143)           # bytes per channel at DSD64: the second and third call end before the next frame exists

with open(os.path.join(GOLDEN, "cascade_digests.json")) as _f:
    DIGESTS = json.load(_f)
with open(os.path.join(GOLDEN, "route_cascade.json")) as _f:
    ROUTE_NAMES = {k: v for v, ks in json.load(_f) for k in ks}


# ---- references: computed once, shared, never changed -----------------------------------------------------------------------------------
_REF = {}


def reference(O, key, kw, bufs, cascade=True):
    """(PCM, frames per call, peaks) of the oracle for a case, by a key of the test's choosing"""
    if key not in _REF:
        pcm, frames, peaks = oracle_run(O, kw, bufs, cascade=cascade)
        pcm.setflags(write=False)
        _REF[key] = (pcm, frames, peaks)
    return _REF[key]


def golden_input(name):
    g = DIGESTS[name]
    kw = g["kw"]
    return kw, call_buffers(make_channels(g["input"]), g["calls"], kw["fmt"], kw["block_size"])


def columns(pcm, kw):
    """the channel subset of an engine out of the oracle's full-width frames"""
    c0, n = kw.get("channel_first", 0), kw.get("channel_count", 0)
    if not n:
        return pcm
    sb = 2 if kw["bit_depth"] == 16 else 4 if kw["bit_depth"] == 32 else 3
    return np.ascontiguousarray(pcm.reshape(-1, kw["channels"], sb)[:, c0:c0 + n]).reshape(-1)


def convert(d, kw, bufs, filt="S", **extra):
    """the calls through d2d_translate on a fresh engine: (PCM, frames per call, peaks, kernel name before, after)"""
    e = d.Engine(filter=filt, **dict(kw, **extra))
    before = e.kernel_name()
    parts, frames = [], []
    for b in bufs:
        pcm, fr = e.translate(b)
        parts.append(pcm.copy())
        frames.append(fr)
    peaks = [e.peak(c) for c in range(e.out_channels)]
    after = e.kernel_name()
    e.close()
    return np.concatenate(parts), frames, peaks, before, after


def route_key(kw, kernel):
    return "%d:%d:S:%d%s24%s:0:0:%d:0" % (kw["dsd_rate"], kw["output_rate"], kw["channels"], kw["fmt"], kw["dither"], kernel)


# ---- 1. every composed pair, every kernel request, both call series -------------------------------------------------------------------

@pytest.mark.parametrize("kernel", [AUTO, LUT, MFMA], ids=["auto", "lut", "mfma"])
@pytest.mark.parametrize("series", ["ragged", "planar"])
@pytest.mark.parametrize("pair", COMPOSED, ids=lambda p: pair_id(*p))
def test_frames_counts_and_peaks_equal_the_oracle_cascade(engine_lib, oracle_mod, pair, series, kernel):
    name = pair_id(*pair) + "_s24_tpdf_" + series
    kw, bufs = golden_input(name)
    want, wfr, wpk = reference(oracle_mod, name, kw, bufs)
    got, fr, pk, before, after = convert(engine_lib, kw, bufs, kernel=kernel)        # (create accepts D2D_KERNEL_MFMA on every pair: route_cascade.json)
    assert fr == wfr == DIGESTS[name]["frames"]
    assert np.array_equal(got, want)
    assert hashlib.sha256(got.tobytes()).hexdigest() == DIGESTS[name]["sha256"] and got[:32 * 6].tobytes().hex() == DIGESTS[name]["head"]
    assert pk == wpk == DIGESTS[name]["peaks"]
    assert [before, after] == ROUTE_NAMES[route_key(kw, kernel)]
    if pair == (2, 96000) and kernel != LUT:
        assert after == "d2d_fir_mfma3_kernel<2, 5, 0, 0, 0>"           # A_M16 through the pipelined int8 kernel's scratch flavour: reached by 'S' only


@pytest.mark.parametrize("kernel", [AUTO, LUT], ids=["auto", "lut"])
@pytest.mark.parametrize("pair", [(1, 96000), (2, 96000)], ids=lambda p: pair_id(*p))
def test_calls_that_yield_no_frame(engine_lib, oracle_mod, pair, kernel):
    dr, rate = pair
    calls = [n * dr for n in DRIP]
    kw = dict(dsd_rate=dr, output_rate=rate, channels=2, bit_depth=24, dither="T", seed=3, **IL)
    bufs = call_buffers([random_bytes(sum(calls), 70 + c) for c in range(2)], calls, "I", 1)
    want, wfr, wpk = reference(oracle_mod, ("drip", pair), kw, bufs)
    assert wfr[0] == 1 and wfr[1] == wfr[2] == 0 and wfr[4] > 30
    got, fr, pk, _, _ = convert(engine_lib, kw, bufs, kernel=kernel)
    assert fr == wfr and np.array_equal(got, want) and pk == wpk


# ---- 2. / 3. formats ------------------------------------------------------------------------------------------------------------------
FORMATS = {
    "mono": dict(channels=1, bit_depth=24, dither="T", **PL),
    "mono_il": dict(channels=1, bit_depth=16, dither="T", **IL),
    "six_planar": dict(channels=6, bit_depth=24, dither="T", **PL),
    "eight_il": dict(channels=8, bit_depth=24, dither="T", **IL),
    "stereo_il_msb": dict(channels=2, bit_depth=24, dither="R", **IL),
    "stereo_planar_msb": dict(channels=2, bit_depth=24, dither="T", fmt="P", endianness="M", block_size=512),
    "s16_tpdf": dict(channels=2, bit_depth=16, dither="T", **PL),
    "s20_rect": dict(channels=2, bit_depth=20, dither="R", **IL),
    "s24_none": dict(channels=2, bit_depth=24, dither="X", **PL),
    "f32_fpd": dict(channels=2, bit_depth=32, dither="F", **IL),
    "f32_none": dict(channels=2, bit_depth=32, dither="X", **PL),
    "s16_rect_il": dict(channels=2, bit_depth=16, dither="R", **IL),
    "s20_tpdf_planar": dict(channels=2, bit_depth=20, dither="T", **PL),
    "s24_m3db": dict(channels=2, bit_depth=24, dither="T", level_db=-3.0, **IL),
    "f32_m3db": dict(channels=2, bit_depth=32, dither="X", level_db=-3.0, **PL),
    "s24_ns": dict(channels=2, bit_depth=24, dither="N", **PL),
    "s16_ns_il": dict(channels=2, bit_depth=16, dither="N", **IL),
    "subset_2_of_8": dict(channels=8, bit_depth=24, dither="T", channel_first=2, channel_count=2, **IL),
}


@pytest.mark.parametrize("fid", sorted(FORMATS))
@pytest.mark.parametrize("pair", [(1, 96000), (2, 96000), (2, 192000)], ids=lambda p: pair_id(*p))
def test_formats(engine_lib, oracle_mod, pair, fid):
    dr, rate = pair
    kw = dict(FORMATS[fid], dsd_rate=dr, output_rate=rate, seed=300 + sorted(FORMATS).index(fid))
    calls = ragged_calls(dr) if kw["fmt"] == "I" else list(PLANAR)
    bufs = call_buffers(make_channels(recipe_for(kw["channels"], sum(calls), dr, kw["endianness"] == "M", 500)), calls, kw["fmt"], kw["block_size"])
    want, wfr, wpk = reference(oracle_mod, ("fmt", pair, fid), kw, bufs)
    got, fr, pk, _, after = convert(engine_lib, kw, bufs)
    c0, n = kw.get("channel_first", 0), kw.get("channel_count", 0) or kw["channels"]
    assert fr == wfr and sum(fr) > 1000
    assert np.array_equal(got, columns(want, kw))
    assert pk == wpk[c0:c0 + n]
    assert "px" not in after and "poly" not in after


# ---- 4. the two definitions side by side -----------------------------------------------------------------------------------------------

def test_s_and_e_differ_where_e_is_composed_each_equal_to_its_oracle(engine_lib, oracle_mod):
    name = "dsd64_192k_s24_tpdf_ragged"
    kw, bufs = golden_input(name)
    want_s, fr_s, _ = reference(oracle_mod, name, kw, bufs)
    want_e, fr_e, _ = reference(oracle_mod, (name, "E"), kw, bufs, cascade=False)
    got_s, gfr_s, _, _, name_s = convert(engine_lib, kw, bufs, filt="S")
    got_e, gfr_e, _, _, name_e = convert(engine_lib, kw, bufs, filt="E")
    assert gfr_s == fr_s == fr_e == gfr_e
    assert np.array_equal(got_s, want_s) and np.array_equal(got_e, want_e)
    assert not np.array_equal(got_s, got_e)
    assert name_e.startswith("d2d_fir_px_kernel<") and name_s.startswith("d2d_fir_mfma3_kernel<1,")


@pytest.mark.parametrize("series", ["ragged", "planar"])
@pytest.mark.parametrize("pair", CONTROL, ids=lambda p: pair_id(*p))
def test_s_and_e_are_the_same_bytes_where_e_is_two_stage(engine_lib, oracle_mod, pair, series):
    name = pair_id(*pair) + "_s24_tpdf_" + series
    kw, bufs = golden_input(name)
    want, wfr, wpk = reference(oracle_mod, name, kw, bufs)
    plain, pfr, ppk = reference(oracle_mod, (name, "E"), kw, bufs, cascade=False)
    assert np.array_equal(want, plain) and wfr == pfr and wpk == ppk
    s, e = convert(engine_lib, kw, bufs, filt="S"), convert(engine_lib, kw, bufs, filt="E")
    assert np.array_equal(s[0], want) and np.array_equal(e[0], want)
    assert s[1:] == e[1:] and s[1] == wfr and s[2] == wpk
    assert hashlib.sha256(s[0].tobytes()).hexdigest() == DIGESTS[name]["sha256"]


# ---- 5. time slices ---------------------------------------------------------------------------------------------------------------------
SLICE_PAIRS = [(1, 96000), (2, 384000)]


class Stream:
    """one stereo planar stream of random bytes (the idle history differs from the true one), the oracle's conversion of all of it and F(p)"""

    def __init__(self, O, pair):
        dr, rate = pair
        self.kw = dict(dsd_rate=dr, output_rate=rate, channels=2, bit_depth=24, dither="T", seed=17, **PL)
        self.L = 16384 + 8 * 147 * dr + 5
        self.chans = [random_bytes(self.L, 900 + 10 * dr + c) for c in range(2)]
        self.want, fr, self.peaks = reference(O, ("slices", pair), self.kw, [self.pack(0, self.L)])
        self.frames = fr[0]
        self._o0 = O.Oracle(**dict(self.kw, filter="E"))              # never fed: max_frames of a fresh context is F (the same under both definitions)

    def pack(self, a, z):
        return pack_layout([c[a:z] for c in self.chans], "P", 4096)

    def F(self, p):
        return self._o0.max_frames(p)

    def rows(self, a, z):
        return self.want[self.F(a) * 6:self.F(z) * 6]


_STREAMS = {}


def stream_of(O, pair):
    if pair not in _STREAMS:
        _STREAMS[pair] = Stream(O, pair)
    return _STREAMS[pair]


@pytest.mark.parametrize("pair", SLICE_PAIRS, ids=lambda p: pair_id(*p))
def test_seek_and_prime_reproduce_the_uninterrupted_conversion(engine_lib, oracle_mod, pair):
    st = stream_of(oracle_mod, pair)
    dr = pair[0]
    e = engine_lib.Engine(filter="S", **st.kw)
    twin = engine_lib.Engine(filter="E", **dict(st.kw, dsd_rate=4, output_rate=96000))       # what an existing cascade engine answers
    assert e.slice_align_bytes() == twin.slice_align_bytes() == 1
    info = e.info()
    pre = e.preroll_bytes()
    assert pre == info["ntaps"] // 8 + (info["P"] + 1) * dr                    # stage A's window plus P + 1 stage-A outputs, as for DSD256 -> 96 kHz
    assert twin.preroll_bytes() == twin.info()["ntaps"] // 8 + (twin.info()["P"] + 1) * 4
    twin.close()
    whole, fr = e.translate(st.pack(0, st.L))
    assert fr == st.frames == st.F(st.L) and np.array_equal(whole, st.want)
    cycle = 147 * dr                                                          # bytes per channel of one L/147 cycle
    for begin in (40 * cycle, 8192, 8192 + 1, 41 * cycle + dr):               # a whole number of cycles, a block edge, odd positions
        q = begin - pre
        e.seek(q)
        assert e.tell() == (q, st.F(q))
        e.prime(st.pack(q, begin))
        assert e.tell() == (begin, st.F(begin)) and [e.peak(c) for c in range(2)] == [0.0, 0.0]
        pcm, n = e.translate(st.pack(begin, st.L))
        assert n == st.frames - st.F(begin) and np.array_equal(pcm, st.rows(begin, st.L)), begin
        assert e.tell() == (st.L, st.frames)
    # control: without the halo the first frames are not the stream's
    e.seek(40 * cycle)
    pcm, n = e.translate(st.pack(40 * cycle, st.L))
    assert not np.array_equal(pcm, st.rows(40 * cycle, st.L))
    e.close()


@pytest.mark.parametrize("pair", SLICE_PAIRS, ids=lambda p: pair_id(*p))
def test_shard_time_slices_concatenate_to_the_single_engine(engine_lib, oracle_mod, pair):
    from dsd2dxd_amd.shard import shard_time
    st = stream_of(oracle_mod, pair)
    parts, names = [], []
    for rank in range(2):
        e = engine_lib.Engine(filter="S", **st.kw)
        halo, begin, end = shard_time(st.L, 2, rank, align=4096 * e.slice_align_bytes(), preroll=e.preroll_bytes())     # a DSF file: cut at its blocks
        assert halo % 4096 == 0 and begin % 4096 == 0 and end > begin and (rank == 0 or begin - halo >= e.preroll_bytes())
        e.seek(halo)
        if begin > halo:
            e.prime(st.pack(halo, begin))
        pcm, n = e.translate(st.pack(begin, end))
        assert n == st.F(end) - st.F(begin)
        parts.append(pcm.copy())
        names.append(e.kernel_name())
        e.close()
    single = convert(engine_lib, st.kw, [st.pack(0, st.L)])
    assert np.array_equal(np.concatenate(parts), single[0]) and np.array_equal(single[0], st.want)
    assert names == [single[4]] * 2


# ---- 6. a device batch on a caller's stream -----------------------------------------------------------------------------------------------

def test_three_unequal_files_on_a_non_blocking_stream(engine_lib, oracle_mod):
    import torch
    d = engine_lib
    kw = dict(dsd_rate=1, output_rate=96000, channels=2, bit_depth=24, dither="T", seed=23, **PL)
    lens = [(4096 * 3, 4096 + 40), (4096, 1177), (8192, 0)]                   # per file: two calls (planar: whole blocks until a stream's last call)
    chans = [[random_bytes(sum(l), 400 + 2 * f + c) for c in range(2)] for f, l in enumerate(lens)]
    cut = lambda f, i: pack_layout([c[sum(lens[f][:i]):sum(lens[f][:i + 1])] for c in chans[f]], "P", 4096)
    refs = [reference(oracle_mod, ("batch", f), kw, [cut(f, 0), cut(f, 1)]) for f in range(3)]
    e = d.Engine(n_files=3, filter="S", **kw)
    s = torch.cuda.Stream()                                                    # (torch creates its streams non-blocking)
    got = [[] for _ in range(3)]
    for i in range(2):
        ios = (d.FileIO * 3)()
        d_in = [torch.from_numpy(cut(f, i)).cuda() if lens[f][i] else None for f in range(3)]
        d_out = []
        for f in range(3):
            n = e.next_frames(lens[f][i], file=f)
            assert n == refs[f][1][i]
            d_out.append(torch.zeros((n * 6 + 31) // 16 * 16, dtype=torch.uint8, device="cuda"))
            ios[f].dsd = d_in[f].data_ptr() if lens[f][i] else None
            ios[f].bytes_per_channel = lens[f][i]
            ios[f].pcm = d_out[f].data_ptr(); ios[f].pcm_capacity_bytes = n * 6
        torch.cuda.synchronize()                                               # the uploads and fills ran on torch's own stream
        e.translate_batch_device(ios, s.cuda_stream)
        s.synchronize()
        for f in range(3):
            assert ios[f].frames_out == refs[f][1][i], (f, i)
            got[f].append(d_out[f][:ios[f].frames_out * 6].cpu().numpy())
    for f in range(3):
        assert np.array_equal(np.concatenate(got[f]), refs[f][0]), f
        assert [e.peak(c, file=f) for c in range(2)] == refs[f][2]
    e.close()


# ---- 7. containment -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pair", [(1, 96000), (2, 96000)], ids=lambda p: pair_id(*p))
def test_only_the_reported_frames_are_written(engine_lib, oracle_mod, pair):
    """the ragged series through d2d_translate_batch_device with pcm_capacity_bytes = frames * 6 exactly and a guard of 4 KiB (more than a tile of
    either stage: 512 stereo 24-bit frames are 3 KiB) in front of and behind every call's frames; twice, on complementary fills"""
    import torch
    d = engine_lib
    name = pair_id(*pair) + "_s24_tpdf_ragged"
    kw, bufs = golden_input(name)
    want, wfr, _ = reference(oracle_mod, name, kw, bufs)
    pattern = np.resize(np.random.default_rng(0xCA5C).integers(0, 256, 4093, dtype=np.uint8), 2 * GUARD + max(wfr) * 6 + 16)
    for comp in (False, True):
        e = d.Engine(filter="S", **kw)
        at = 0
        for b, n in zip(bufs, wfr):
            size = 2 * GUARD + ((n * 6 + 15) & ~15)
            fill = (~pattern if comp else pattern)[:size].copy()
            arena, d_in = torch.from_numpy(fill.copy()).cuda(), torch.from_numpy(b).cuda()
            ios = (d.FileIO * 1)()
            ios[0].dsd = d_in.data_ptr(); ios[0].bytes_per_channel = b.size // 2
            ios[0].pcm = arena.data_ptr() + GUARD; ios[0].pcm_capacity_bytes = n * 6
            e.translate_batch_device(ios, torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            after = arena.cpu().numpy()
            assert ios[0].frames_out == n
            assert np.array_equal(after[GUARD:GUARD + n * 6], want[at:at + n * 6]), (comp, n)
            assert np.array_equal(after[:GUARD], fill[:GUARD]), (comp, n, "front guard")
            assert np.array_equal(after[GUARD + n * 6:], fill[GUARD + n * 6:]), (comp, n, "behind the frames")
            at += n * 6
        e.close()


# ---- 8. the table blob ------------------------------------------------------------------------------------------------------------------

def test_tables_blob_moves_between_s_engines_and_not_between_definitions(engine_lib, oracle_mod):
    import torch
    d = engine_lib
    name = "dsd64_96k_s24_tpdf_planar"
    kw, bufs = golden_input(name)
    want, wfr, _ = reference(oracle_mod, name, kw, bufs)
    s1, s2, e1 = d.Engine(filter="S", **kw), d.Engine(filter="S", **kw), d.Engine(filter="E", **kw)
    cap = max(s1.tables_bytes(), e1.tables_bytes())
    blob_s = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    blob_e = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    s1.tables_export_device(blob_s.data_ptr(), cap)
    e1.tables_export_device(blob_e.data_ptr(), cap)
    torch.cuda.synchronize()
    assert blob_s[28:32].cpu().numpy().view("<u4")[0] == ord("A") and blob_e[28:32].cpu().numpy().view("<u4")[0] == ord("P")      # TableBlobHeader.filter_type
    s2.tables_import_device(blob_s.data_ptr(), cap)
    for eng, blob in ((s2, blob_e), (e1, blob_s)):
        with pytest.raises(d.D2DError) as ei:
            eng.tables_import_device(blob.data_ptr(), cap)
        assert ei.value.code == -1 and "does not match" in ei.value.message
    for eng in (s2, s1):                                                       # the importer, refusals behind it, converts like the exporter
        got = np.concatenate([eng.translate(b)[0].copy() for b in bufs])
        assert np.array_equal(got, want)
    plain = reference(oracle_mod, (name, "E"), kw, bufs, cascade=False)[0]
    assert np.array_equal(np.concatenate([e1.translate(b)[0].copy() for b in bufs]), plain)
    for eng in (s1, s2, e1):
        eng.close()


# ---- 9. FLAC ----------------------------------------------------------------------------------------------------------------------------

def test_verified_flac_stream_decodes_to_the_oracle_cascade(engine_lib, oracle_mod):
    d = engine_lib
    nbytes = 4096 * 10                                                         # 11146 frames at 96 kHz: two whole FLAC blocks and a short one
    chans = [synth("sine", nbytes, seed=3), synth("pink", nbytes, seed=4, amp=0.098)]
    kw = dict(dsd_rate=1, output_rate=96000, channels=2, bit_depth=24, dither="T", seed=9, **PL)
    want, wfr, _ = reference(oracle_mod, "flac", kw, [pack_layout(chans, "P", 4096)])
    pos, out = [0], []

    def read(cap):
        a = pos[0]
        b = min(nbytes, a + cap)
        pos[0] = b
        return pack_layout([c[a:b] for c in chans], "P", 4096).tobytes() if b > a else b""

    e = d.Engine(filter="S", **kw)
    stats, chk = e.convert_stream_flac(read, out.append, total_bytes_per_channel=nbytes, chunk_bytes_per_channel=3 * 4096, effort=1, verify=True)
    e.close()
    assert stats.samples_per_channel == wfr[0] == 11146 and stats.blocks == 3
    pcm, n, dchk = d.flac_decode_host(2, 24, b"".join(out))
    assert n == wfr[0] and np.array_equal(np.frombuffer(pcm, dtype=np.uint8), want)


# ---- 10. the host driver ----------------------------------------------------------------------------------------------------------------

def test_cli_convert_and_levels_with_t_s(engine_lib, oracle_mod, tmp_path):
    from test_host_driver import _wav_payload
    if not os.path.exists(CLI):
        engine_lib.build_library()
    n = 4096 * 4 + 700
    chans = [synth("sine", n, seed=5, amp=0.5), synth("pink", n, seed=6, amp=0.098)]
    src = str(tmp_path / "tone.dsf")
    write_dsf(src, chans, dsd_rate=1, lsb_first=True)
    buf = [pack_layout(chans, "P", 4096)]
    base = dict(dsd_rate=1, output_rate=96000, channels=2, seed=0, **PL)
    want, wfr, _ = reference(oracle_mod, "cli", dict(base, bit_depth=24, dither="T"), buf)
    for sub in ("s", "e"):
        (tmp_path / sub).mkdir()
    subprocess.check_call([CLI, "convert", "-t", "S", "-r", "96000", "-o", "W", "-b", "24", "-d", "T", "-p", str(tmp_path / "s"), "-q", src])
    fmt, pay = _wav_payload(str(tmp_path / "s" / "tone.wav"))
    assert fmt[:4] == (1, 2, 96000, 96000 * 6) and np.array_equal(pay, want)
    subprocess.check_call([CLI, "convert", "-r", "96000", "-o", "W", "-b", "24", "-d", "T", "-p", str(tmp_path / "e"), "-q", src])
    assert not np.array_equal(_wav_payload(str(tmp_path / "e" / "tone.wav"))[1], pay)            # (-t E, the default: the composed definition)
    # levels: the peak of the float conversion without dither
    o = oracle_mod.Oracle(**dict(base, filter="E", bit_depth=32, dither="X"))
    o.use_cascade()
    o.translate(buf[0])
    out = subprocess.check_output([CLI, "levels", "-t", "S", "-r", "96000", src]).decode().splitlines()
    assert out[0] == "tone.dsf: %.4f dBFS" % float(o.peak_dbfs()) and out[1] == "Highest peak: %.4f dBFS" % float(o.peak_dbfs())
    p = subprocess.run([CLI, "convert", "-t", "S", "-r", "88200", "-o", "W", "-p", str(tmp_path / "s"), "-q", src], stderr=subprocess.PIPE)
    assert p.returncode == 1 and b"48 kHz multiples only" in p.stderr


# ---- 11. d2d_get_info -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pair", COMPOSED + CONTROL, ids=lambda p: pair_id(*p))
def test_info_names_stage_a_and_stage_b(engine_lib, pair):
    d = engine_lib
    dr, rate = pair
    with open(os.path.join(ROOT, "filters", "filter_tables.json")) as f:
        tables = json.load(f)
    fa, = [x for x in tables["filters"] if x["name"] == "A_M%d" % (8 * dr)]
    rb, = [x for x in tables["resamplers"] if x["out_rate"] == rate]
    e = d.Engine(filter="S", dsd_rate=dr, output_rate=rate, channels=2, bit_depth=24, dither="T", **PL)
    i = d.Info()
    assert d.lib().d2d_get_info(e._h, C.byref(i)) == 0
    assert (i.decimation, i.ntaps, i.scale_bits) == (8 * dr, fa["N"], fa["S"])
    assert (i.resamp_L, i.resamp_M, i.resamp_P) == (rb["L"], 147, rb["P"]) and rb["L"] * 2400 == rate
    assert i.filter_name == fa["name"].encode() and i.abi_version == 11 and i.kernel == MFMA
    e.close()


def test_s_is_refused_before_any_device_work_at_a_44k_rate(engine_lib):
    with pytest.raises(engine_lib.D2DError) as ei:
        engine_lib.Engine(filter="S", dsd_rate=1, output_rate=88200, channels=2, bit_depth=24, dither="T", device=99, **PL)
    assert ei.value.code == -3 and "48 kHz multiples only" in ei.value.message       # D2D_ERR_FILTER, not the device error of ordinal 99
