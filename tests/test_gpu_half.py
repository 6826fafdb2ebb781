"""The halved engine on the GPU (d2d_create_half) against tests/half_ref.py, and the half pass on its own
(d2d_half_frames_device) against its CPU twin.

Streams yield about 6000 sums per channel and reach the engine in ragged calls through d2d_translate_batch_device with exact capacities:
one call yields an odd number of sums, one fewer than NT - 1, one none at all, one crosses two of the kernel's blocks (1024 frames each),
one takes the rest.  After every call d2d_tell and the frames delivered are held to (n + 1) >> 1 of the sums the stream holds.
  (a) every rate, filter, depth and dither of the issue's list against the reference, bytes and peaks;
  (b) a batch of three files of different lengths, one empty, on a caller's non-blocking stream;
  (c) d2d_seek + d2d_prime slices at both parities of the sum count equal the uninterrupted conversion, frames and peak;
  (d) containment: a guarded arena with exact capacities under two complementary fills, and a D2D_ERR_CAPACITY refusal that changes nothing;
  (e) the pass alone at int32 extremes, on ties, and at n = 0, 1, 2 and one block +- 1."""
import ctypes as C

import numpy as np
import pytest

import half_ref
from helpers import decode_pcm, pack_layout, random_bytes, synth

gpu = pytest.mark.gpu
Q, T = half_ref.taps()
NT = len(Q)
H = NT - 1
BLOCK = 1024                                            # frames of one block of d2d_half_kernel (frames of at most 64 bytes)
IMAX = (1 << 31) - 1
BASE = dict(dsd_rate=1, output_rate=44100, channels=2, fmt="P", endianness="L", block_size=4096, filter="E", bit_depth=24, dither="T", seed=5)

SHAPES = {
    "dsd64_44k1_stereo_24T": dict(),
    "dsd128_44k1_mono_16R": dict(dsd_rate=2, channels=1, bit_depth=16, dither="R"),
    "dsd256_44k1_stereo_floatF": dict(dsd_rate=4, bit_depth=32, dither="F"),
    "dsd64_48k_three_20X": dict(output_rate=48000, channels=3, bit_depth=20, dither="X"),
    "dsd128_48k_stereo_24T": dict(dsd_rate=2, output_rate=48000),
    "xld_dsd64_44k1_24R": dict(filter="X", dither="R"),
    "chebyshev_dsd128_44k1_16T": dict(dsd_rate=2, filter="C", bit_depth=16),
    "interleaved_msb_stereo": dict(fmt="I", endianness="M"),
    "minus3dB_24T": dict(level_db=-3.0),
    "plus6dB_16T_clipping": dict(level_db=6.0, bit_depth=16),
}


def sums_after(kw, p):
    """sums a stream holds after p bytes per channel: the FIR outputs of the doubled rate (48 kHz: of the composed 96 kHz filter, which
    exist as soon as the two stages 352.8 kHz -> x 40 / 147 would have produced them)"""
    if kw["output_rate"] == 44100:
        return p // (2822400 * kw["dsd_rate"] // 88200 // 8)
    nfir = p // kw["dsd_rate"]
    return (nfir * 40 - 1) // 147 + 1 if nfir else 0


def bytes_for(kw, n):
    """the fewest bytes per channel after which a stream holds n sums"""
    p = 0
    step = 1 << 20
    while step:
        while sums_after(kw, p + step) < n:
            p += step
        step >>= 1
    return p + 1 if n else 0


def channels_of(n, nbytes, seed, dsd_rate=1, amp=0.352):
    out = []
    for c in range(n):
        out.append(synth("sine", nbytes, seed=seed + c, freq=700.0 * (c + 1), dsd_rate=dsd_rate, amp=amp) if c % 2 == 0 else
                   synth("pink", nbytes, seed=seed + c, amp=0.3, dsd_rate=dsd_rate))
    return out


def okw_of(kw):
    return {k: kw[k] for k in ("dsd_rate", "output_rate", "channels", "fmt", "endianness", "block_size", "filter")}


def epi_of(kw):
    return dict(bit_depth=kw["bit_depth"], dither=kw["dither"], level_db=kw.get("level_db", 0.0), seed=kw["seed"])


def scale_of(kw):
    return half_ref.SCALE[(kw["dsd_rate"], kw["output_rate"], kw["filter"])]


def ragged_cuts(kw, total_sums):
    """byte positions of the calls' ends, and the checks that the calls are what the docstring says"""
    a = bytes_for(kw, 1001)
    b = bytes_for(kw, 1001 + 100)
    c = b + 1
    d = bytes_for(kw, 1101 + 2 * 2 * BLOCK + 301)
    cuts = [a, b, c, d, bytes_for(kw, total_sums)]
    n = [sums_after(kw, p) for p in [0] + cuts]
    per_call = [y - x for x, y in zip(n, n[1:])]
    assert per_call[0] % 2 == 1 and 0 < per_call[1] < H and per_call[2] == 0 and per_call[3] > 2 * 2 * BLOCK and per_call[4] > 0, per_call
    assert 3000 <= n[-1] <= 20000
    return cuts


def convert(d, e, kw, files, cuts, stream=None, check_tell=True):
    """files[f]: channels of file f (a file that has run out feeds 0 bytes).  Every call through d2d_translate_batch_device with exact
    capacities.  Returns the bytes per file."""
    import torch
    n = len(files)
    outs = [[] for _ in range(n)]
    keep = []
    pos = [0] * n
    prev = 0
    for cut in cuts:
        ios = (d.FileIO * n)()
        planned = []
        for f, ch in enumerate(files):
            z = min(cut, ch[0].size)
            piece = [c[pos[f]:z] for c in ch]
            L = piece[0].size
            buf = pack_layout(piece, kw["fmt"], kw["block_size"]) if L else np.zeros(0, dtype=np.uint8)
            t_in = torch.from_numpy(np.concatenate([buf, np.zeros(16, dtype=np.uint8)])).cuda()
            nfr = e.next_frames(L, file=f)
            want_frames = half_ref.frames_after(sums_after(kw, z)) - half_ref.frames_after(sums_after(kw, pos[f]))
            assert nfr == want_frames, (f, cut, nfr, want_frames)
            t_out = torch.full((max(nfr * e.frame_bytes, 16),), 0xA5, dtype=torch.uint8, device="cuda")
            ios[f].dsd, ios[f].bytes_per_channel, ios[f].pcm, ios[f].pcm_capacity_bytes = t_in.data_ptr(), L, t_out.data_ptr(), nfr * e.frame_bytes
            keep.append(t_in)
            outs[f].append((t_out, nfr))
            planned.append(nfr)
            pos[f] = z
        torch.cuda.synchronize()
        e.translate_batch_device(ios, stream)
        assert [ios[f].frames_out for f in range(n)] == planned
        if check_tell:
            for f in range(n):
                assert e.tell(f) == (pos[f], half_ref.frames_after(sums_after(kw, pos[f]))), (f, cut)
        prev = cut
    assert prev == cuts[-1]
    for f in range(n):
        e.peak(0, file=f)                                # (waits for the engine's stream)
    torch.cuda.synchronize()
    fb = e.frame_bytes
    return [np.concatenate([t.cpu().numpy()[:k * fb] for t, k in o] + [np.zeros(0, dtype=np.uint8)]) for o in outs]


def peaks_of(e, f=0):
    return [e.peak(c, file=f) for c in range(e.out_channels)]


def first_difference(got, want):
    return int(np.flatnonzero(got != want)[0]) if got.size == want.size else ("sizes", got.size, want.size)


# ---- (a) every shape against the reference ----

@gpu
@pytest.mark.parametrize("name", list(SHAPES))
def test_engine_against_the_reference(engine_lib, oracle_mod, name):
    d = engine_lib
    kw = dict(BASE, **SHAPES[name])
    total = 6100
    cuts = ragged_cuts(kw, total)
    chans = channels_of(kw["channels"], cuts[-1], seed=20, dsd_rate=kw["dsd_rate"], amp=0.7 if kw.get("level_db", 0.0) > 0 else 0.352)
    S = scale_of(kw)
    want, wpk, X = half_ref.stream_frames(oracle_mod, okw_of(kw), [pack_layout(chans, kw["fmt"], kw["block_size"])], S, **epi_of(kw))
    assert X.shape[1] == total
    e = d.Engine.create_half(**kw)
    try:
        assert e.half_factor() == 2 and e.info()["S"] == S
        sb = 2 if kw["bit_depth"] == 16 else 4 if kw["bit_depth"] == 32 else 3
        assert e.frame_bytes == kw["channels"] * sb
        got = convert(d, e, kw, [chans], cuts)[0]
        assert got.size == half_ref.frames_after(total) * e.frame_bytes
        assert np.array_equal(got, want), first_difference(got, want)
        assert peaks_of(e) == list(wpk)
        if kw.get("level_db", 0.0) > 0:
            v = decode_pcm(got, 16, 2)
            assert v.max() == (1 << 15) - 1 and v.min() == -(1 << 15)             # clipped at both ends
        # d2d_reset: the same stream again gives the same bytes
        e.reset()
        assert e.tell() == (0, 0) and peaks_of(e) == [0.0] * kw["channels"]
        again = convert(d, e, kw, [chans], [cuts[0], cuts[-1]])[0]
        assert np.array_equal(again, want)
    finally:
        e.close()


# ---- (b) a batch on a caller's non-blocking stream ----

@gpu
def test_batch_of_three_files_on_a_callers_stream(engine_lib, oracle_mod):
    from test_gpu_inflight import hip_runtime
    d = engine_lib
    kw = dict(BASE)
    cuts = ragged_cuts(kw, 6100)
    lengths = [cuts[-1], 0, bytes_for(kw, 3001)]
    files = [channels_of(2, n, seed=40 + 10 * f) if n else [np.zeros(0, dtype=np.uint8)] * 2 for f, n in enumerate(lengths)]
    L = hip_runtime()
    h = C.c_void_p()
    assert L.hipStreamCreateWithFlags(C.byref(h), 1) == 0 and h.value           # hipStreamNonBlocking
    e = d.Engine.create_half(n_files=3, **kw)
    try:
        e.profile_enable(True)
        got = convert(d, e, kw, files, cuts, stream=h.value)
        fir_ms, step_ms, launches = e.profile_read_all()
        assert launches >= 4 and step_ms > fir_ms > 0.0                          # `step` includes the half pass
        for f in (0, 2):
            want, wpk, _ = half_ref.stream_frames(oracle_mod, okw_of(kw), [pack_layout(files[f], "P", 4096)], scale_of(kw), **epi_of(kw))
            assert np.array_equal(got[f], want), (f, first_difference(got[f], want))
            assert peaks_of(e, f) == list(wpk), f
        assert got[1].size == 0 and peaks_of(e, 1) == [0.0, 0.0] and e.tell(1) == (0, 0)
    finally:
        e.close()
        assert L.hipStreamDestroy(h) == 0


# ---- (c) seek + prime slices ----

@gpu
@pytest.mark.parametrize("rate", [44100, 48000])
def test_seek_and_prime_slices_equal_the_uninterrupted_conversion(engine_lib, oracle_mod, rate):
    d = engine_lib
    kw = dict(BASE, output_rate=rate)
    S = scale_of(kw)
    nbytes = bytes_for(kw, 5000)
    chans = channels_of(2, nbytes, seed=70)
    X = half_ref.sums_at(oracle_mod, okw_of(kw), [pack_layout(chans, "P", 4096)], S)
    e = d.Engine.create_half(**kw)
    try:
        whole, n = e.translate(pack_layout(chans, "P", 4096))
        whole = whole.copy()
        want, wpk = half_ref.half_frames(oracle_mod, X, S, **epi_of(kw))
        assert np.array_equal(whole, want) and peaks_of(e) == list(wpk)
        fb, pre = e.frame_bytes, e.preroll_bytes()
        assert e.slice_align_bytes() == 1 and 1400 <= pre <= 6400
        seen = set()
        for target in (2000, 2001, 3333, 3334):
            p = bytes_for(kw, target) + 1
            np_ = sums_after(kw, p)
            seen.add(np_ % 2)
            q = p - pre
            assert q > 0
            e.seek(q)
            e.prime(pack_layout([c[q:p] for c in chans], "P", 4096))
            assert e.tell() == (p, half_ref.frames_after(np_)) and peaks_of(e) == [0.0, 0.0]      # a prime produces no frames and moves no peak
            first = e.tell()[1]
            part, m = e.translate(pack_layout([c[p:] for c in chans], "P", 4096))
            assert first + m == n and np.array_equal(part, whole[first * fb:]), (target, first_difference(part, whole[first * fb:]))
            # the peak is that of exactly those frames: the reference's, on the sums from n(p) on with the H before them
            _, ppk = half_ref.half_frames(oracle_mod, X[:, np_:], S, first=np_, hist=X[:, np_ - H:np_], **epi_of(kw))
            assert peaks_of(e) == list(ppk), target
        assert seen == {0, 1}
        e.seek(0)
        again, _ = e.translate(pack_layout(chans, "P", 4096))
        assert np.array_equal(again, whole) and peaks_of(e) == list(wpk)
    finally:
        e.close()


# ---- (d) containment, and a refusal that changes nothing ----

@gpu
@pytest.mark.parametrize("complement", [False, True])
def test_only_the_reported_frames_are_written(engine_lib, oracle_mod, complement):
    from test_gpu_containment import GUARD, Layout
    d = engine_lib
    kw = dict(BASE)
    e = d.Engine.create_half(n_files=3, **kw)
    fb = e.frame_bytes
    assert fb == 6 and BLOCK * fb <= GUARD
    try:
        lengths = (bytes_for(kw, 2 * 2 * BLOCK + 803), 0, bytes_for(kw, 2 * BLOCK + 23))
        files = [channels_of(2, n, seed=90 + f) if n else [np.zeros(0, dtype=np.uint8)] * 2 for f, n in enumerate(lengths)]
        inputs = [pack_layout(ch, "P", 4096) if ch[0].size else np.zeros(0, dtype=np.uint8) for ch in files]
        nfr = [e.next_frames(ch[0].size, file=f) for f, ch in enumerate(files)]
        assert (nfr[0] * fb) % 16 and (nfr[2] * fb) % 16 and nfr[1] == 0 and nfr[0] > 2 * BLOCK     # ragged tails, more than two blocks
        lay = Layout(d, "device", inputs, [n * fb for n in nfr], complement)
        for f, ch in enumerate(files):
            lay.ios[f].bytes_per_channel = ch[0].size
        lay.ios[2].pcm_capacity_bytes = nfr[2] * fb - 1
        with pytest.raises(d.D2DError) as ei:
            e.translate_batch_device(lay.ios)
        assert ei.value.code == -20
        lay.check([None, None, None], fb, "refused call")
        assert [e.tell(f) for f in range(3)] == [(0, 0)] * 3 and all(peaks_of(e, f) == [0.0, 0.0] for f in range(3))
        lay.ios[2].pcm_capacity_bytes = nfr[2] * fb
        e.translate_batch_device(lay.ios)
        assert [lay.ios[f].frames_out for f in range(3)] == nfr
        want = [half_ref.stream_frames(oracle_mod, okw_of(kw), [inputs[f]], scale_of(kw), **epi_of(kw))[0] if nfr[f] else None for f in range(3)]
        lay.check(want, fb, "halved call")
        lay2 = Layout(d, "device", inputs, [64, 64, 64], complement)             # a prime writes nothing
        for f, ch in enumerate(files):
            lay2.ios[f].bytes_per_channel = ch[0].size
        e.prime_batch_device(lay2.ios)
        lay2.check([None, None, None], fb, "prime")
    finally:
        e.close()


# ---- (e) the pass on its own ----

def _device_equals_host(d, lines, firsts, S, **epi):
    """d2d_half_frames_device on the lines (each (channels, H + n) int32) against the twin: bytes and peaks; the output sits between guards"""
    import torch
    want = d.half_frames_host(lines, firsts, S, **epi)
    channels = lines[0].shape[0]
    jobs = (d.HalfJob * len(lines))()
    keep = []
    GUARD_B = 4096
    for j, x, first, (wb, _) in zip(jobs, lines, firsts, want):
        t_x = torch.from_numpy(np.ascontiguousarray(x, dtype=np.int32)).cuda()
        t_o = torch.full((GUARD_B + wb.size + GUARD_B,), 0x5A, dtype=torch.uint8, device="cuda")
        t_p = torch.zeros(channels, dtype=torch.float64, device="cuda")
        assert (t_o.data_ptr() + GUARD_B) % 16 == 0
        j.sums, j.stride, j.n, j.first_index = t_x.data_ptr(), x.shape[1], x.shape[1] - H, first
        j.pcm, j.pcm_capacity_bytes, j.peaks = t_o.data_ptr() + GUARD_B, wb.size, t_p.data_ptr()
        keep.append((t_x, t_o, t_p))
    torch.cuda.synchronize()
    d.half_frames_device(jobs, channels, S, **epi)
    for i, ((t_x, t_o, t_p), (wb, wp)) in enumerate(zip(keep, want)):
        o = t_o.cpu().numpy()
        assert jobs[i].frames_out * channels * (2 if epi["bit_depth"] == 16 else 4 if epi["bit_depth"] == 32 else 3) == wb.size
        assert np.all(o[:GUARD_B] == 0x5A) and np.all(o[GUARD_B + wb.size:] == 0x5A), i
        got = o[GUARD_B:GUARD_B + wb.size]
        assert np.array_equal(got, wb), (i, first_difference(got, wb))
        assert np.array_equal(t_p.cpu().numpy(), wp), i
    return want


def _line(new, hist=None):
    new = np.atleast_2d(np.asarray(new, dtype=np.int64))
    hist = np.zeros((new.shape[0], H), dtype=np.int64) if hist is None else np.atleast_2d(np.asarray(hist, dtype=np.int64))
    return np.concatenate([hist, new], axis=1).astype(np.int32)


@gpu
def test_pass_alone_at_int32_extremes_and_ties(engine_lib):
    d = engine_lib
    n = 2 * BLOCK * 2 + 2 * NT
    lines, firsts = [], []
    for sign in (1, -1):
        new = np.zeros(n, dtype=np.int64)
        for c in (NT + 1, 2 * BLOCK + NT + 1):                                   # one window in the first block, one in the second
            for j in range(NT):
                new[c - j] = sign * (IMAX if Q[j] >= 0 else -IMAX)
        lines.append(_line(np.stack([new, -new]))); firsts.append(0)
        tie = np.zeros(n, dtype=np.int64)
        tie[NT + 10] = sign << (T - 1)
        tie[2 * BLOCK + 77] = -sign << (T - 1)
        lines.append(_line(np.stack([tie, tie[::-1].copy()]))); firsts.append(1 if sign > 0 else 0)
    rng = np.random.default_rng(3)
    lines.append(rng.integers(-(1 << 31), 1 << 31, (2, H + n), dtype=np.int64).astype(np.int32)); firsts.append((1 << 33) - 2 * BLOCK - 1)
    for bits, dither, S in ((24, "T", 30), (32, "X", 0), (16, "R", 30), (32, "F", 28), (20, "X", 29)):
        want = _device_equals_host(d, lines, firsts, S, bit_depth=bits, dither=dither, seed=9)
        if bits == 24:
            assert want[0][1][0] > 4.9 and want[2][1][1] > 4.9                   # |w| 2^-30 = sum |q| (2^31 - 1) 2^-26 2^-30 = 4.95, either sign


@gpu
def test_pass_alone_at_the_smallest_sizes_and_block_edges(engine_lib):
    d = engine_lib
    rng = np.random.default_rng(4)
    sizes = [0, 1, 2, 3, 2 * BLOCK - 2, 2 * BLOCK - 1, 2 * BLOCK, 2 * BLOCK + 1, 2 * BLOCK + 2]
    for channels, bits, dither in ((2, 24, "T"), (1, 16, "R"), (3, 32, "F"), (64, 32, "X")):
        lines, firsts = [], []
        for n in sizes:
            for first in (0, 1):
                lines.append(rng.integers(-(1 << 31), 1 << 31, (channels, H + n), dtype=np.int64).astype(np.int32)); firsts.append(first)
        if channels == 64:                                                        # (256-byte frames: blocks of 256 frames; a few blocks each)
            lines, firsts = lines[6:12], firsts[6:12]
        _device_equals_host(d, lines, firsts, 29, bit_depth=bits, dither=dither, seed=2, level_db=-2.0)
