"""The mixed engine on the GPU (d2d_create_mix), against tests/mix_ref.py and against the unmixed engine.

Inputs are a few tiles long and reach the engine in three ragged calls through d2d_translate_batch_device with exact capacities: one call
ends past a tile edge on a length that is no multiple of anything, one yields a single frame, one takes the rest.
  (a) 32768 I gives the plain engine's bytes and peaks, one shape per FIR family;
  (b) the 5.1 and 5.0 presets and a signed permutation against the reference, three files of different lengths in one batch, one empty;
  (c) a row at the sum |m| bound on streams that attain the table's extreme sums;
  (d) d2d_seek + d2d_prime slices equal the uninterrupted conversion;
  (e) containment: a guarded arena with exact capacities, and a D2D_ERR_CAPACITY refusal that changes nothing;
  (f) the three calls enqueued back to back on a caller's non-blocking stream."""
import numpy as np
import pytest

import adversarial
import mix_ref
from helpers import pack_layout, random_bytes, synth

gpu = pytest.mark.gpu
U = mix_ref.UNITY
TILE = {8: 512, 16: 512, 32: 576, 64: 384}          # outputs per wave-tile of the FIR kernels (tests/adversarial.py: FIR_TILE); 96 kHz: 480 = 160 x 3 groups


def channels_of(n, nbytes, seed, dsd_rate=1):
    """n channels of distinct material: tones, pink noise, random bits"""
    out = []
    for c in range(n):
        k = c % 3
        out.append(synth("sine", nbytes, seed=seed + c, freq=500.0 * (c + 1), dsd_rate=dsd_rate) if k == 0 else
                   synth("pink", nbytes, seed=seed + c, amp=0.3, dsd_rate=dsd_rate) if k == 1 else random_bytes(nbytes, seed + c))
    return out


class Batch:
    """n files through d2d_translate_batch_device, call by call, every buffer a device tensor with the exact capacity"""

    def __init__(self, d, e, kw):
        self.d, self.e, self.kw, self.n = d, e, kw, e.n_files
        self.out = [[] for _ in range(self.n)]
        self.keep = []

    def pack(self, chans):
        return pack_layout(chans, self.kw["fmt"], self.kw.get("block_size", 4096)) if chans[0].size else np.zeros(0, dtype=np.uint8)

    def plan(self, pieces):
        """pieces[f]: the call's channels of file f (equal lengths, 0 allowed) -> (ios, output tensors, frame counts)"""
        import torch
        ios = (self.d.FileIO * self.n)()
        outs, frames = [], []
        for f, chans in enumerate(pieces):
            buf = self.pack(chans)
            L = chans[0].size
            t_in = torch.from_numpy(np.concatenate([buf, np.zeros(16, dtype=np.uint8)])).cuda()
            nfr = self.e.next_frames(L, file=f)
            t_out = torch.full((max(nfr * self.e.frame_bytes, 16),), 0xA5, dtype=torch.uint8, device="cuda")
            ios[f].dsd, ios[f].bytes_per_channel, ios[f].pcm, ios[f].pcm_capacity_bytes = t_in.data_ptr(), L, t_out.data_ptr(), nfr * self.e.frame_bytes
            self.keep.append(t_in)
            outs.append(t_out); frames.append(nfr)
        return ios, outs, frames

    def call(self, pieces, stream=None, prime=False):
        import torch
        ios, outs, frames = self.plan(pieces)
        torch.cuda.synchronize()
        (self.e.prime_batch_device if prime else self.e.translate_batch_device)(ios, stream)
        if prime:
            return
        assert [ios[f].frames_out for f in range(self.n)] == frames
        for f in range(self.n):
            self.out[f].append((outs[f], frames[f]))

    def result(self):
        import torch
        torch.cuda.synchronize()
        fb = self.e.frame_bytes
        return [np.concatenate([t.cpu().numpy()[:n * fb] for t, n in o] + [np.zeros(0, dtype=np.uint8)]) for o in self.out]


def convert_ragged(d, e, kw, files, tile_bytes, stream=None):
    """files[f]: channels of file f (lengths may differ, 0 allowed), in three calls; a file that has run out feeds 0 bytes.
    Returns the Batch (result(): the bytes per file)."""
    b = Batch(d, e, kw)
    n = len(files)
    pos = [0] * n
    # call 1: past the first tile edge, ragged (a short file gives what it has)
    first = [min(tile_bytes + 37, ch[0].size) for ch in files]
    b.call([[c[:first[f]] for c in files[f]] for f in range(n)], stream)
    pos = first
    # call 2: the shortest call that yields ONE frame for file 0; the others get the same length (or what they have left)
    one = next(L for L in range(1, 4096) if e.next_frames(L, file=0) == 1)
    second = [min(one, files[f][0].size - pos[f]) for f in range(n)]
    b.call([[c[pos[f]:pos[f] + second[f]] for c in files[f]] for f in range(n)], stream)
    assert b.out[0][-1][1] == 1
    pos = [p + s for p, s in zip(pos, second)]
    # call 3: the rest
    b.call([[c[pos[f]:] for c in files[f]] for f in range(n)], stream)
    return b


def peaks_of(e, f=0):
    return [e.peak(c, file=f) for c in range(e.out_channels)]


# ---- (a) the identity mix equals the plain engine ----

BASE = dict(dsd_rate=1, output_rate=88200, channels=2, fmt="P", endianness="L", block_size=4096, filter="E", bit_depth=24, dither="T", seed=5)
IDENTITY_SHAPES = {
    "stereo_88k2_24T": dict(),
    "six_88k2": dict(channels=6),
    "five_planar": dict(channels=5),
    "mono": dict(channels=1),
    "dsd128_352k8_16R": dict(dsd_rate=2, output_rate=352800, bit_depth=16, dither="R"),
    "96k_E": dict(output_rate=96000),
    "float_F_minus3dB": dict(bit_depth=32, dither="F", level_db=-3.0),
    "interleaved_msb_stereo": dict(fmt="I", endianness="M"),
    "interleaved_lsb_six": dict(fmt="I", channels=6),
    "interleaved_lsb_four_96k": dict(fmt="I", channels=4, output_rate=96000),
    "planar_msb_three": dict(endianness="M", channels=3),
    "lut_three": dict(channels=3, kernel=1),
}


def tile_bytes_of(kw):
    if kw["output_rate"] % 44100:
        return 480 * (2822400 * kw["dsd_rate"] // 8) // kw["output_rate"] + 1
    M = 2822400 * kw["dsd_rate"] // kw["output_rate"]
    return TILE[M] * M // 8


@gpu
@pytest.mark.parametrize("name", list(IDENTITY_SHAPES))
def test_identity_mix_equals_the_plain_engine(engine_lib, name):
    d = engine_lib
    kw = dict(BASE, **IDENTITY_SHAPES[name])
    C_, tb = kw["channels"], tile_bytes_of(kw)
    chans = channels_of(C_, 3 * tb + 1234, seed=20, dsd_rate=kw["dsd_rate"])
    plain, mixed = d.Engine(**kw), d.Engine(mix=mix_ref.identity(C_), **kw)
    try:
        assert mixed.get_mix() == mix_ref.identity(C_) and plain.get_mix() is None
        assert mixed.frame_bytes == plain.frame_bytes and mixed.out_channels == C_
        want = convert_ragged(d, plain, kw, [chans], tb).result()[0]
        got = convert_ragged(d, mixed, kw, [chans], tb).result()[0]
        assert want.size > 2 * 480 * plain.frame_bytes
        assert np.array_equal(got, want), int(np.flatnonzero(got != want)[0]) if got.size == want.size else (got.size, want.size)
        assert peaks_of(mixed) == peaks_of(plain) and mixed.tell() == plain.tell()
        assert mixed.peak_dbfs() == plain.peak_dbfs()
    finally:
        plain.close(); mixed.close()


# ---- (b) presets and a signed permutation against the reference ----

MIXES = {
    "5_1": (6, lambda d: d.mix_preset(6, 2)),
    "5_0": (5, lambda d: d.mix_preset(5, 2)),
    "5_1_mono": (6, lambda d: d.mix_preset(6, 1)),
    "signed_permutation": (3, lambda d: [[0, 0, -U], [U, 0, 0], [0, -U, 0]]),
}
FORMATS = {"88k2_24T": dict(), "96k_24T": dict(output_rate=96000), "352k8_float": dict(output_rate=352800, bit_depth=32, dither="F", level_db=-3.0)}


def reference(O, kw, chans, coef):
    okw = {k: kw[k] for k in ("dsd_rate", "output_rate", "channels", "fmt", "endianness", "block_size", "filter")}
    X, S = mix_ref.exact_sums(O, okw, [pack_layout(chans, kw["fmt"], kw["block_size"])])
    return mix_ref.mix_frames(O, X, S, coef, bit_depth=kw["bit_depth"], dither=kw["dither"], level_db=kw.get("level_db", 0.0), seed=kw["seed"])


@gpu
@pytest.mark.parametrize("fmt", list(FORMATS))
@pytest.mark.parametrize("mix", list(MIXES))
def test_mixes_against_the_reference_in_a_batch(engine_lib, oracle_mod, mix, fmt):
    d = engine_lib
    C_, make = MIXES[mix]
    coef = make(d)
    kw = dict(BASE, channels=C_, **FORMATS[fmt])
    tb = tile_bytes_of(kw)
    lengths = [2 * tb + 777, tb + 300, 0]                               # three files of different lengths, one of them empty
    files = [channels_of(C_, n, seed=40 + 10 * f) if n else [np.zeros(0, dtype=np.uint8)] * C_ for f, n in enumerate(lengths)]
    e = d.Engine(n_files=3, mix=coef, **kw)
    try:
        assert e.out_channels == len(coef) and e.frame_bytes == len(coef) * (4 if kw["bit_depth"] == 32 else 3)
        got = convert_ragged(d, e, kw, files, tb).result()
        for f in range(2):
            want, wpk = reference(oracle_mod, kw, files[f], coef)
            assert got[f].size == want.size and np.array_equal(got[f], want), (f, int(np.flatnonzero(got[f][:want.size] != want[:got[f].size])[0]))
            assert peaks_of(e, f) == list(wpk), f
        assert got[2].size == 0 and peaks_of(e, 2) == [0.0] * len(coef) and e.tell(2) == (0, 0)
        with pytest.raises(d.D2DError):
            e.peak(len(coef), file=0)                                   # d2d_peak: channel < Co
    finally:
        e.close()


# ---- (c) the bound-saturating row on adversarial streams ----

@gpu
def test_row_at_the_bound_on_worst_case_streams(engine_lib, oracle_mod):
    d = engine_lib
    st = adversarial.build_for(1, 88200, T=64)
    one = st.packed()[:4 * 576 * 4 + 1000]                              # the first windows: a few tiles
    coef = [[1 << 17] * 16, [(-1) ** c * (1 << 17) for c in range(16)], [1 << 17] * 8 + [-(1 << 17)] * 7 + [0]]
    for bits, dither in ((24, "T"), (32, "F")):
        kw = dict(BASE, channels=16, bit_depth=bits, dither=dither)
        e = d.Engine(mix=coef, **kw)
        try:
            got = convert_ragged(d, e, kw, [[one] * 16], 576 * 4).result()[0]
            want, wpk = reference(oracle_mod, kw, [one] * 16, coef)
            assert np.array_equal(got, want) and peaks_of(e) == list(wpk)
            assert wpk[0] > 32.0                                         # far beyond full scale: the integer depths clip
            if bits == 24:
                from helpers import decode_pcm
                v = decode_pcm(got, 24, 3)
                assert v[:, 0].max() == (1 << 23) - 1 and v[:, 0].min() == -(1 << 23)
        finally:
            e.close()


# ---- (d) seek + prime slices ----

@gpu
@pytest.mark.parametrize("fmt", ["88k2_24T", "96k_24T"])
def test_seek_and_prime_slices_equal_the_uninterrupted_conversion(engine_lib, fmt):
    d = engine_lib
    kw = dict(BASE, channels=6, **FORMATS[fmt])
    coef = d.mix_preset(6, 2)
    tb = tile_bytes_of(kw)
    chans = channels_of(6, 3 * tb + 555, seed=70)
    e = d.Engine(mix=coef, **kw)
    try:
        whole, n = e.translate(pack_layout(chans, "P", 4096))
        whole, pk_whole = whole.copy(), peaks_of(e)
        fb, pre = e.frame_bytes, e.preroll_bytes()
        assert e.slice_align_bytes() == 1
        for p in (tb + 13, 2 * tb + 1):
            q = max(0, p - pre)
            e.seek(q)
            e.prime(pack_layout([c[q:p] for c in chans], "P", 4096))
            assert e.tell()[0] == p and peaks_of(e) == [0.0, 0.0]       # a prime produces no frames and moves no peak
            first = e.tell()[1]
            part, m = e.translate(pack_layout([c[p:] for c in chans], "P", 4096))
            assert first + m == n and np.array_equal(part, whole[first * fb:])
        e.seek(0)
        again, _ = e.translate(pack_layout(chans, "P", 4096))
        assert np.array_equal(again, whole) and peaks_of(e) == pk_whole
    finally:
        e.close()


# ---- (e) containment ----

@gpu
@pytest.mark.parametrize("complement", [False, True])
def test_only_the_reported_frames_are_written(engine_lib, oracle_mod, complement):
    from test_gpu_containment import GUARD, Layout
    d = engine_lib
    kw = dict(BASE, channels=6)
    coef = d.mix_preset(6, 2)
    tb = tile_bytes_of(kw)
    e = d.Engine(n_files=3, mix=coef, **kw)
    fb = e.frame_bytes
    assert fb == 6 and 576 * 4 * fb <= GUARD
    try:
        files = [channels_of(6, n, seed=90 + f) if n else [np.zeros(0, dtype=np.uint8)] * 6 for f, n in enumerate((2 * tb + 401, 0, tb + 11))]
        inputs = [pack_layout(ch, "P", 4096) if ch[0].size else np.zeros(0, dtype=np.uint8) for ch in files]
        nfr = [e.next_frames(ch[0].size, file=f) for f, ch in enumerate(files)]
        assert (nfr[0] * fb) % 16 and (nfr[2] * fb) % 16 and nfr[1] == 0   # ragged tails: the last 16-byte piece of a file is partial
        # a buffer one byte short: D2D_ERR_CAPACITY, and no byte, no position, no peak changes
        lay = Layout(d, "device", inputs, [n * fb for n in nfr], complement)
        for f, ch in enumerate(files):
            lay.ios[f].bytes_per_channel = ch[0].size
        lay.ios[2].pcm_capacity_bytes = nfr[2] * fb - 1
        with pytest.raises(d.D2DError) as ei:
            e.translate_batch_device(lay.ios)
        assert ei.value.code == -20
        lay.check([None, None, None], fb, "refused call")
        assert [e.tell(f) for f in range(3)] == [(0, 0)] * 3 and all(peaks_of(e, f) == [0.0, 0.0] for f in range(3))
        # the call itself: exactly the Co-wide frames
        lay.ios[2].pcm_capacity_bytes = nfr[2] * fb
        e.translate_batch_device(lay.ios)
        assert [lay.ios[f].frames_out for f in range(3)] == nfr
        want = [reference(oracle_mod, kw, files[f], coef)[0] if nfr[f] else None for f in range(3)]
        lay.check(want, fb, "mixed call")
        # a prime writes nothing
        lay2 = Layout(d, "device", inputs, [64, 64, 64], complement)
        for f, ch in enumerate(files):
            lay2.ios[f].bytes_per_channel = ch[0].size
        e.prime_batch_device(lay2.ios)
        lay2.check([None, None, None], fb, "prime")
    finally:
        e.close()


# ---- (f) a caller's non-blocking stream ----

@gpu
def test_calls_enqueued_back_to_back_on_a_callers_stream(engine_lib, oracle_mod):
    import ctypes as C
    import torch
    from test_gpu_inflight import hip_runtime
    d = engine_lib
    kw = dict(BASE, channels=6)
    coef = d.mix_preset(6, 2)
    tb = tile_bytes_of(kw)
    files = [channels_of(6, 2 * tb + 999, seed=110), channels_of(6, tb + 77, seed=120)]
    L = hip_runtime()
    h = C.c_void_p()
    assert L.hipStreamCreateWithFlags(C.byref(h), 1) == 0 and h.value           # hipStreamNonBlocking
    e = d.Engine(n_files=2, mix=coef, **kw)
    try:
        e.profile_enable(True)
        # every buffer exists, filled, before the first call (capacities by an upper bound: the exact counts need the engine's position);
        # then the three calls go out one after the other with nothing in between
        fb = e.frame_bytes
        cuts = [(0, tb + 37), (tb + 37, tb + 37 + 4), (tb + 37 + 4, None)]
        calls = []
        for a, z in cuts:
            ios, outs = (d.FileIO * 2)(), []
            for f, ch in enumerate(files):
                piece = [c[a:z] for c in ch]
                t_in = torch.from_numpy(np.concatenate([pack_layout(piece, "P", 4096), np.zeros(16, dtype=np.uint8)])).cuda()
                cap = (piece[0].size // 4 + 2) * fb
                t_out = torch.full(((cap + 15) // 16 * 16,), 0xA5, dtype=torch.uint8, device="cuda")
                ios[f].dsd, ios[f].bytes_per_channel, ios[f].pcm, ios[f].pcm_capacity_bytes = t_in.data_ptr(), piece[0].size, t_out.data_ptr(), cap
                outs.append((t_in, t_out))
            calls.append((ios, outs))
        torch.cuda.synchronize()
        for ios, _ in calls:
            e.translate_batch_device(ios, h.value)
        outs = [([o[1] for o in os_], [ios[f].frames_out for f in range(2)]) for ios, os_ in calls]
        assert outs[1][1][0] == 1                                                # the middle call: a single frame
        assert torch.cuda.ExternalStream(h.value).query() in (True, False)
        pk = [peaks_of(e, f) for f in range(2)]                                  # d2d_peak waits for the engine's stream
        fir_ms, step_ms, launches = e.profile_read_all()
        assert launches == 3 and step_ms > fir_ms > 0.0                          # `step` includes the mix pass
        torch.cuda.synchronize()
        for f in range(2):
            got = np.concatenate([o[f].cpu().numpy()[:n[f] * e.frame_bytes] for o, n in outs])
            want, wpk = reference(oracle_mod, kw, files[f], coef)
            assert np.array_equal(got, want) and pk[f] == list(wpk)
    finally:
        e.close()
        assert L.hipStreamDestroy(h) == 0
