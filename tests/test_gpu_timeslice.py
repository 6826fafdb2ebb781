"""Time slices (d2d_seek / d2d_prime, include/dsd2dxd_amd.h): an engine that is sought to a position and primed with a short halo
produces byte for byte the frames of an uninterrupted conversion from there on -- on every kernel route, at odd cut points, for
slices converted out of order on one engine.  The expected bytes of a slice [a, b) are rows F(a) .. F(b) of the oracle's
conversion of the whole stream (the oracle is a streaming context and needs no seek).

Streams are random bytes: the idle history must differ from the true one, or a missing halo would be invisible (the control
test below shows that it is not)."""
import ctypes as C

import numpy as np
import pytest

from helpers import pack_layout, random_bytes

pytestmark = pytest.mark.gpu

PL = dict(fmt="P", endianness="L", block_size=4096)
IM = dict(fmt="I", endianness="M", block_size=1)
NBYTES, CUTS = 24776, (40, 16411)          # 40 lies inside every preroll (the halo clamps to 0); 16411 is odd and no multiple of any Mb

# id -> (engine / oracle parameters, cut points or None for the defaults)
CASES = {
    "c01_fp6_frames": (dict(dsd_rate=1, output_rate=88200, channels=2, bit_depth=24, dither="T", **PL), None),
    "c02_il2_s16_gain": (dict(dsd_rate=1, output_rate=88200, channels=2, bit_depth=16, dither="T", level_db=-3.0, **IM), None),
    "c03_mono_pair": (dict(dsd_rate=1, output_rate=88200, channels=1, bit_depth=24, dither="T", **PL), (8192, 16384 + 1)),
    "c04_int8_m8": (dict(dsd_rate=1, output_rate=352800, channels=2, bit_depth=24, dither="T", **PL), None),
    "c05_lut": (dict(dsd_rate=1, output_rate=176400, channels=2, bit_depth=24, dither="T", kernel=1, **IM), None),
    "c06_poly_il2": (dict(dsd_rate=1, output_rate=96000, channels=2, bit_depth=24, dither="T", **IM), None),
    "c07_poly_mono": (dict(dsd_rate=2, output_rate=384000, channels=1, bit_depth=16, dither="R", **PL), None),
    "c08_cascade": (dict(dsd_rate=4, output_rate=96000, channels=2, bit_depth=24, dither="T", **PL), None),
    "c09_config5": (dict(dsd_rate=8, output_rate=96000, channels=8, bit_depth=24, dither="T", **IM), None),
    "c10_channel_subset": (dict(dsd_rate=1, output_rate=88200, channels=6, bit_depth=24, dither="T", channel_first=2, channel_count=2, **IM), None),
    "c11_taps32_two_pass": (dict(dsd_rate=1, output_rate=88200, channels=1, bit_depth=24, dither="T", tap_bits=32, **PL), None),
    "c12_taps32_one_pass": (dict(dsd_rate=1, output_rate=88200, channels=2, bit_depth=24, dither="T", tap_bits=32, **PL), None),
    # noise-shaped: frames can only start at a multiple of 8192, i.e. at multiples of A = slice_align_bytes(); L = 2 A + 4000, cuts at A and 2 A
    "c13_ns_44k": (dict(dsd_rate=1, output_rate=88200, channels=2, bit_depth=16, dither="N", **PL), "A"),
    "c14_ns_48k": (dict(dsd_rate=1, output_rate=96000, channels=2, bit_depth=24, dither="N", **IM), "A"),
}
NS_ALIGN = {"c13_ns_44k": (32768, 4), "c14_ns_48k": (150528, 1)}       # (A, Mb)


class Ref:
    """one case's stream, the oracle's conversion of it and an uninterrupted engine's: computed once, shared, never changed"""

    def __init__(self, cid, d, O):
        kw, cuts = CASES[cid]
        self.kw = dict(kw, filter="E", seed=1000 + sorted(CASES).index(cid))
        okw = {k: v for k, v in self.kw.items() if k not in ("kernel", "channel_first", "channel_count")}
        self.c0 = kw.get("channel_first", 0)
        self.nch = kw.get("channel_count", 0) or kw["channels"]
        if cuts == "A":
            A = NS_ALIGN[cid][0]
            self.L, self.cuts = 2 * A + 4000, (A, 2 * A)
        else:
            self.L, self.cuts = NBYTES, cuts or CUTS
        self.chans = [random_bytes(self.L, 50 * sorted(CASES).index(cid) + c) for c in range(kw["channels"])]
        o = O.Oracle(**okw)
        self._o0 = O.Oracle(**okw)                       # never fed: orc_max_frames of a fresh context is F
        self._O = O
        want, fr = o.translate(self.pack(0, self.L))
        sb = o.frame_bytes // kw["channels"]
        self.fb = sb * self.nch
        self.want = np.ascontiguousarray(want[:fr * o.frame_bytes].reshape(fr, kw["channels"], sb)[:, self.c0:self.c0 + self.nch]).reshape(-1)
        self.frames = fr
        self.opeaks = [o.peak(self.c0 + c) for c in range(self.nch)]
        e = d.Engine(**self.kw)
        whole, wfr = e.translate(self.pack(0, self.L))
        assert wfr == fr == self.F(self.L)
        self.whole = whole.copy()
        self.wpeaks = [e.peak(c) for c in range(self.nch)]
        self.wname = e.kernel_name()
        e.close()

    def F(self, p):
        """frames an uninterrupted conversion has produced after p bytes per channel"""
        return self._O.lib().orc_max_frames(self._o0._h, p)

    def pack(self, a, z):
        """the call buffer that feeds bytes [a, z) of every channel"""
        return pack_layout([c[a:z] for c in self.chans], self.kw["fmt"], self.kw["block_size"])

    def rows(self, a, z=None):
        return self.want[self.F(a) * self.fb:(self.F(z) * self.fb if z is not None else None)]


_REFS = {}


def ref_of(cid, d, O):
    if cid not in _REFS:
        _REFS[cid] = Ref(cid, d, O)
    return _REFS[cid]


def convert_slice(e, ref, begin, end, halo=None):
    """seek(halo_begin) -> prime -> translate of [begin, end) on engine e; checks tell() and the peaks on the way"""
    q = max(0, begin - e.preroll_bytes()) if halo is None else halo
    e.seek(q)
    assert e.tell() == (q, ref.F(q))
    if begin > q:
        e.prime(ref.pack(q, begin))
    assert e.tell() == (begin, ref.F(begin))
    assert [e.peak(c) for c in range(ref.nch)] == [0.0] * ref.nch          # a prime meters nothing
    pcm, fr = e.translate(ref.pack(begin, end))
    assert fr == ref.F(end) - ref.F(begin)
    assert e.tell() == (end, ref.F(end))
    return pcm.copy(), [e.peak(c) for c in range(ref.nch)]


@pytest.mark.parametrize("cid", sorted(CASES))
def test_slices_out_of_order_equal_the_uninterrupted_conversion(engine_lib, oracle_mod, cid):
    ref = ref_of(cid, engine_lib, oracle_mod)
    e = engine_lib.Engine(**ref.kw)
    assert 0 < e.preroll_bytes() <= 4096
    if cid in NS_ALIGN:
        assert e.slice_align_bytes() == NS_ALIGN[cid][0]
    else:
        assert e.slice_align_bytes() == 1
    p1, p2 = ref.cuts
    bounds = [(0, p1), (p1, p2), (p2, ref.L)]
    got, peaks = {}, {}
    for i in (2, 0, 1):                                   # deliberately shuffled, on ONE engine
        got[i], peaks[i] = convert_slice(e, ref, *bounds[i])
        assert np.array_equal(got[i], ref.rows(*bounds[i])), f"slice {i}"
    name = e.kernel_name()
    cat = np.concatenate([got[0], got[1], got[2]])
    assert ref.frames > 0 and cat.size == ref.frames * ref.fb
    assert np.array_equal(cat, ref.whole)
    assert np.array_equal(ref.whole, ref.want)
    for c in range(ref.nch):
        assert max(peaks[i][c] for i in range(3)) == ref.wpeaks[c] == ref.opeaks[c]
    assert name == ref.wname
    e.close()


def test_mono_pair_on_a_primed_history_row(engine_lib, oracle_mod):
    """c03's slices behind a prime have odd lengths and take the ordinary mono kernel; an even slice behind a prime takes the pair route, whose
    first half reads the primed history row"""
    ref = ref_of("c03_mono_pair", engine_lib, oracle_mod)
    e = engine_lib.Engine(**ref.kw)
    for begin, end in ((8192, 16384), (16384 + 8, 16384 + 8 + 4096)):
        pcm, _ = convert_slice(e, ref, begin, end)
        assert np.array_equal(pcm, ref.rows(begin, end)), begin
        assert e.kernel_name() != ref.wname                  # (the whole stream's length is no multiple of 32: that engine ran the ordinary mono kernel)
    fresh = engine_lib.Engine(**ref.kw)
    fresh.translate(ref.pack(0, 8192))
    assert e.kernel_name() == fresh.kernel_name()
    fresh.close()
    e.close()


@pytest.mark.parametrize("cid", sorted(NS_ALIGN))
def test_noise_shaped_slices_start_on_segment_boundaries(engine_lib, oracle_mod, cid):
    ref = ref_of(cid, engine_lib, oracle_mod)
    A, Mb = NS_ALIGN[cid]
    e = engine_lib.Engine(**ref.kw)
    assert e.slice_align_bytes() == A
    for k in (1, 2, 3):
        e.seek(k * A)
        assert e.tell()[0] == k * A and e.tell()[1] % 8192 == 0 and e.tell()[1] > 0
    # one decimation step past a boundary: the shaper's state there is unknown to a sought engine
    e.seek(A + Mb)
    assert e.tell()[1] % 8192 != 0
    with pytest.raises(engine_lib.D2DError) as ei:
        e.translate(ref.pack(A + Mb, 2 * A))
    assert ei.value.code == -40 and "8192" in ei.value.message           # D2D_ERR_STATE
    assert e.tell() == (A + Mb, ref.F(A + Mb))                            # ... and nothing changed
    # primed up to a position that is no boundary: still refused
    e.seek(A)
    e.prime(ref.pack(A, A + Mb))
    with pytest.raises(engine_lib.D2DError) as ei:
        e.translate(ref.pack(A + Mb, 2 * A))
    assert ei.value.code == -40
    # the engine still converts: the middle slice, then on from where it stands (no seek: the state is carried)
    pcm, _ = convert_slice(e, ref, A, 2 * A)
    assert np.array_equal(pcm, ref.rows(A, 2 * A))
    tail, _ = e.translate(ref.pack(2 * A, ref.L))
    assert np.array_equal(tail, ref.rows(2 * A))
    # an engine that was never sought may cut anywhere
    e.seek(0)
    a, _ = e.translate(ref.pack(0, A + Mb))
    b, _ = e.translate(ref.pack(A + Mb, 2 * A))
    assert np.array_equal(np.concatenate([a, b]), ref.rows(0, 2 * A))
    e.close()


@pytest.mark.parametrize("cid", ["c01_fp6_frames", "c06_poly_il2", "c08_cascade"])
def test_control_a_missing_halo_shows(engine_lib, oracle_mod, cid):
    """seek with NO prime: the first frames differ from the uninterrupted conversion's (idle history instead of the stream's), the
    frames behind the preroll are its frames again"""
    ref = ref_of(cid, engine_lib, oracle_mod)
    e = engine_lib.Engine(**ref.kw)
    p2 = ref.cuts[1]
    e.seek(p2)
    got, fr = e.translate(ref.pack(p2, ref.L))
    want = ref.rows(p2)
    assert got.size == want.size == fr * ref.fb
    n_pre = ref.F(p2 + e.preroll_bytes()) - ref.F(p2) + 2
    assert 0 < n_pre < fr
    assert not np.array_equal(got[:n_pre * ref.fb], want[:n_pre * ref.fb])
    assert np.array_equal(got[n_pre * ref.fb:], want[n_pre * ref.fb:])
    e.close()


def test_a_halo_of_exactly_the_preroll_is_enough(engine_lib, oracle_mod):
    """the cascade has the longest chain (bit window -> P + 1 stage-A outputs -> frame): begin - halo_begin == preroll_bytes() exactly, at
    cuts on and off the stage-A grid"""
    ref = ref_of("c08_cascade", engine_lib, oracle_mod)
    e = engine_lib.Engine(**ref.kw)
    pre = e.preroll_bytes()
    for begin in (pre, 9001, 16384, 16411, 16412, 16413):
        pcm, _ = convert_slice(e, ref, begin, ref.L, halo=begin - pre)
        assert np.array_equal(pcm, ref.rows(begin)), begin
    e.close()


def test_batch_one_file_seeks_the_others_carry_on(engine_lib, oracle_mod):
    import torch
    d = engine_lib
    kw = dict(dsd_rate=1, output_rate=88200, channels=2, bit_depth=24, dither="T", filter="E", seed=77, **PL)
    L, cut, p = NBYTES, 8192, 16411
    chans = [[random_bytes(L, 900 + 2 * f + c) for c in range(2)] for f in range(3)]
    pack = lambda f, a, z: pack_layout([c[a:z] for c in chans[f]], "P", 4096)
    wants, opeaks, osamples = [], [], []
    for f in range(3):
        o = oracle_mod.Oracle(**kw)
        w, fr, y = o.translate(pack(f, 0, L), want_f64=True)            # y: the samples |.| of which the oracle's peak meter takes
        wants.append(w[:fr * 6])
        opeaks.append([o.peak(c) for c in range(2)])
        osamples.append(y)
    o0 = oracle_mod.Oracle(**kw)
    F = lambda q: oracle_mod.lib().orc_max_frames(o0._h, q)
    e = d.Engine(n_files=3, **kw)
    dev = torch.device("cuda", 0)

    def call(ranges, prime=False):
        """ranges: per file (a, z) or None; returns the frames' bytes per file"""
        ios = (d.FileIO * 3)()
        keep, outs = [], []
        for f, r in enumerate(ranges):
            if r is None:
                outs.append(None)
                continue
            t = torch.from_numpy(pack(f, *r)).to(dev)
            keep.append(t)
            ios[f].dsd = t.data_ptr(); ios[f].bytes_per_channel = r[1] - r[0]
            if not prime:
                n = e.next_frames(r[1] - r[0], file=f)
                out = torch.zeros((n * 6 + 31) // 16 * 16, dtype=torch.uint8, device=dev)
                outs.append(out)
                ios[f].pcm = out.data_ptr(); ios[f].pcm_capacity_bytes = n * 6
        (e.prime_batch_device if prime else e.translate_batch_device)(ios)
        torch.cuda.synchronize()
        if prime:
            assert all(ios[f].frames_out == 0 for f in range(3))
            return None
        return [None if o is None else o[:ios[f].frames_out * 6].cpu().numpy() for f, o in enumerate(outs)]

    first = call([(0, cut)] * 3)
    halo = max(0, p - e.preroll_bytes())
    e.seek(halo, file=1)
    assert [e.tell(f) for f in range(3)] == [(cut, F(cut)), (halo, F(halo)), (cut, F(cut))]
    call([None, (halo, p), None], prime=True)
    assert [e.peak(c, file=1) for c in range(2)] == [0.0, 0.0] and all(e.peak(c, file=f) > 0.0 for f in (0, 2) for c in range(2))
    second = call([(cut, L), (p, L), (cut, L)])
    for f in (0, 2):
        assert np.array_equal(np.concatenate([first[f], second[f]]), wants[f]), f
    assert np.array_equal(first[1], wants[1][:F(cut) * 6])
    assert np.array_equal(second[1], wants[1][F(p) * 6:])
    # file 1's peak is the peak of the frames since its seek (the seek cleared that file's peaks and no other's); the others' of the whole stream
    for f in (0, 2):
        assert [e.peak(c, file=f) for c in range(2)] == opeaks[f]
    since = [float(np.abs(osamples[1][F(p):, c]).max()) for c in range(2)]
    assert [e.peak(c, file=1) for c in range(2)] == since
    e.close()


def test_errors(engine_lib):
    import torch
    d = engine_lib
    L = d.lib()
    e = d.Engine(n_files=2, dsd_rate=1, output_rate=88200, channels=2, bit_depth=24, dither="T", **PL)
    for call in (lambda: e.seek(0, file=2), lambda: e.tell(file=2)):
        with pytest.raises(d.D2DError) as ei:
            call()
        assert ei.value.code == -1                                        # D2D_ERR_PARAM
    pos, fr = C.c_uint64(), C.c_uint64()
    assert L.d2d_seek(None, 0, 0) == -1
    assert L.d2d_tell(None, 0, C.byref(pos), C.byref(fr)) == -1
    assert L.d2d_prime(None, None, 0) == -1
    assert L.d2d_prime_batch_device(None, None, 0, None) == -1
    assert L.d2d_preroll_bytes(None) == 0 and L.d2d_slice_align_bytes(None) == 0
    t = torch.zeros(4096 * 2 + 16, dtype=torch.uint8, device="cuda")
    ios = (d.FileIO * 2)()
    ios[0].dsd = t.data_ptr() + 1; ios[0].bytes_per_channel = 4096
    with pytest.raises(d.D2DError) as ei:
        e.prime_batch_device(ios)
    assert ei.value.code == -1 and "aligned" in ei.value.message
    assert e.tell(0) == (0, 0)
    with pytest.raises(d.D2DError) as ei:                                 # the host-pointer twin is for single-file engines, like d2d_translate
        e.prime(np.zeros(8192, dtype=np.uint8))
    assert ei.value.code == -40
    e.close()
