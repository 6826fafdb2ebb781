"""Every kernel route writes the frames it reports and nothing else (include/dsd2dxd_amd.h: the containment contract next to d2d_file_io).

The parity tests compare the frames a call reports; none of them can see a byte outside those frames: Engine.translate goes through the engine's
own staging, and the device-buffer tests never read their slack.  Here every buffer of a call lies inside an ARENA: one allocation
[guard][file 0][pad to the next 16][file 1]...[guard] with pcm_capacity_bytes = frames * frame_bytes exactly, files back to back as a caller
packs them, a guard of 32 KiB (more than the largest tile of any kernel times the widest frame, asserted per case) on both sides, so that
whatever a kernel could touch one tile beyond its range is inside a live allocation: an overrun is a failed comparison, never a fault.  The
inputs sit in a second arena of the same shape.  Every case runs twice, on a fresh engine and oracle: the first run fills both arenas with a
position-dependent pattern, the second with its complement, so a stray byte cannot equal both fills and an output that depends on a byte
behind the declared input changes between the runs.  After every call: the bytes inside each file's range equal the oracle's, frame counts,
peaks and tell() agree, the kernel is the route's, and every other byte of both arenas is the fill.

  * device batches (d2d_translate_batch_device): every route of tests/test_gpu_long_streams.py with the E filter plus the routes whose tail
    code those do not reach; three files, three calls: whole tiles that end on the file's last byte, counts that are no multiple of the tile,
    one block, calls of 0 bytes, ragged tails whose frame counts cover the residues 1, 2, 3 modulo 4 (a lane takes four frames);
  * the mono pair, whose second half starts wherever the first ends.  A pair needs halves of whole 16-byte chunks and whole outputs, so at
    M = 32 (MONO) a half holds a multiple of four frames and its 24-bit frames end on a multiple of 12 bytes: an ODD first-half count cannot
    occur there.  It can at M = 128 (16 bytes per output): those cases use blocks of 4112 = 16 * 257 bytes, and the second half starts at an
    odd byte (24-bit) or at 2 modulo 4 (16-bit);
  * one long case per pipelined family: every wave walks several tiles in its fixed-order loop, which stores a tile early and rewrites it;
  * the host entry points on pinned and pageable arenas, the staged pipeline with 8192-byte slices, d2d_convert_stream's write callback;
  * d2d_prime_batch_device writes nothing; a call that fails with D2D_ERR_CAPACITY or D2D_ERR_PARAM changes no byte, no position, no peak.

test_checker_* (not marked gpu) cover the checker itself on numpy arrays."""

import numpy as np
import pytest

from helpers import pack_layout, random_bytes
from test_gpu_extreme_sums import DBG_NO_INTQ, DBG_NS_GENERAL, DBG_TAPS32_2PASS, TWO_PASS_KERNEL, tile_of
from test_gpu_long_streams import ENGINE_ONLY, MONO, MONO_KERNEL, NS_ROUTES, PAIR_KERNEL, PL, ROUTES

gpu = pytest.mark.gpu

DBG_NO_COOP, DBG_HOST_STAGED = 1 << 2, 1 << 3          # dsd2dxd_amd/_capi.py (asserted against it in Run)
GUARD = 32 * 1024                                      # the largest tile: 576 outputs x 32 bytes (fp6, 32 * 6 * 3 outputs, eight channels of float) = 18432
NB = 4096                                              # the planar block of the routes (px_kind2: 1024, the odd mono pair: 4112); the nominal one of interleaved routes
LIMIT = 1 << 16                                        # no call of the short cases is longer than this per channel
SUBSET = ("channel_first", "channel_count")            # engine-only too: the oracle converts every channel and the test picks the columns


# ---- the arena and its checker (numpy only) ----

class Arena:
    """[guard][file 0: sizes[0] bytes][pad to the next 16][file 1]...[guard]: where every file starts, and the whole size"""

    def __init__(self, sizes):
        self.sizes = [int(n) for n in sizes]
        self.starts, pos = [], GUARD
        for n in self.sizes:
            self.starts.append(pos)
            pos = (pos + n + 15) & ~15
        self.total = pos + GUARD

    def end(self, i):
        return self.starts[i] + self.sizes[i]


_PATTERN = np.random.default_rng(0xF111).integers(0, 256, 65521, dtype=np.uint8)       # (a prime period: no two 16-byte rows of an arena alike)


def fill_bytes(n, complement):
    """the position-dependent fill of an arena of n bytes, or its bitwise complement"""
    f = np.resize(_PATTERN, n)
    return ~f if complement else f


def violations(arena, got, fill, want):
    """What is wrong with an arena after a call: `got` its bytes now, `fill` its bytes before the call, `want[i]` the bytes file i's range must
    hold (None: untouched).  A list of (place, file, offset, count): place 'front guard' (offset < 0: relative to the file's START, of the
    changed byte nearest to it), 'pad' and 'back guard' (offset >= 0: relative to the file's END, 0 = the first byte behind the file, of the
    first changed byte), 'frames' (offset of the first wrong byte inside the file); count = bytes changed / wrong there."""
    out = []
    n = len(arena.sizes)

    def outside(lo, hi, place, file):
        d = np.flatnonzero(got[lo:hi] != fill[lo:hi])
        if d.size:
            off = lo + int(d[-1]) - arena.starts[0] if place == "front guard" else lo + int(d[0]) - arena.end(file)
            out.append((place, file, off, int(d.size)))

    outside(0, arena.starts[0], "front guard", 0)
    for i in range(n):
        lo, hi = arena.starts[i], arena.end(i)
        ref = fill[lo:hi] if want[i] is None else want[i]
        assert ref.size == hi - lo
        d = np.flatnonzero(got[lo:hi] != ref)
        if d.size:
            out.append(("frames", i, int(d[0]), int(d.size)))
        if i + 1 < n:
            outside(hi, arena.starts[i + 1], "pad", i)
    outside(arena.end(n - 1), arena.total, "back guard", n - 1)
    return out


def describe(v, frame_bytes=None):
    s = []
    for place, f, off, cnt in v:
        if place == "frames":
            at = f"byte {off}" + (f" (frame {off // frame_bytes})" if frame_bytes else "")
            s.append(f"file {f}: {cnt} bytes inside its range are not the expected ones, the first at {at}")
        elif place == "front guard":
            s.append(f"front guard: {cnt} bytes changed, the nearest {-off} bytes before file {f}'s start")
        else:
            s.append(f"{place} behind file {f}: {cnt} bytes changed, the first {off} bytes past the file's end")
    return "; ".join(s)


def test_checker_names_the_place_of_a_stray_byte():
    sizes = [1000, 0, 37, 4096]                      # pads of 8 and 11 bytes; an empty file shares its place with its neighbour
    a = Arena(sizes)
    assert a.starts == [GUARD, GUARD + 1008, GUARD + 1008, GUARD + 1056] and a.total == GUARD + 1056 + 4096 + GUARD
    assert all(s % 16 == 0 for s in a.starts)
    for comp in (False, True):
        fill = fill_bytes(a.total, comp)
        want = [random_bytes(n, 5 + i) if n else None for i, n in enumerate(sizes)]
        clean = fill.copy()
        for i, w in enumerate(want):
            if w is not None:
                clean[a.starts[i]:a.end(i)] = w
        assert violations(a, clean, fill, want) == []
        assert violations(a, fill.copy(), fill, [None] * 4) == []
        for pos, expect in [(a.starts[0] - 1, ("front guard", 0, -1, 1)), (5, ("front guard", 0, 5 - GUARD, 1)),
                            (a.end(0), ("pad", 0, 0, 1)), (a.end(0) + 7, ("pad", 0, 7, 1)), (a.end(2) + 3, ("pad", 2, 3, 1)),
                            (a.end(3), ("back guard", 3, 0, 1)), (a.total - 1, ("back guard", 3, GUARD - 1, 1))]:
            bad = clean.copy()
            bad[pos] ^= 0x40
            assert violations(a, bad, fill, want) == [expect], (pos, expect)
            assert str(abs(expect[2])) in describe([expect]) and expect[0] in describe([expect])
        bad = clean.copy()
        bad[a.starts[2] + 30] ^= 1                   # a wrong byte inside a range, and a file that should have stayed untouched
        bad[a.starts[3] + 100:a.starts[3] + 103] ^= 0xFF
        assert violations(a, bad, fill, want[:3] + [None])[0] == ("frames", 2, 30, 1)
        assert violations(a, bad, fill, want) == [("frames", 2, 30, 1), ("frames", 3, 100, 3)]
        assert "frame 10" in describe([("frames", 3, 60, 2)], 6)


def test_checker_pair_of_fills_catches_a_byte_that_equals_one_fill():
    """a stray store of a constant: where the constant happens to equal the first fill that run sees nothing; the complement run must"""
    a = Arena([256, 256])
    pos = a.end(1) + 2
    stray = fill_bytes(a.total, False)[pos]
    seen = []
    for comp in (False, True):
        fill = fill_bytes(a.total, comp)
        got = fill.copy()
        got[pos] = stray
        seen.append(violations(a, got, fill, [None, None]))
    assert seen[0] == [] and seen[1] == [("back guard", 1, 2, 1)]
    f0, f1 = fill_bytes(1 << 17, False), fill_bytes(1 << 17, True)
    assert np.all(f0 ^ f1 == 0xFF) and f0.dtype == np.uint8 and len(set(f0[:65521:16].tobytes())) > 200


# ---- memory a call can use: device, pinned host, pageable host ----

class Mem:
    def __init__(self, kind, data):
        import torch
        self.kind = kind
        if kind == "device":
            self.t = torch.from_numpy(np.ascontiguousarray(data)).cuda()
            self.ptr = self.t.data_ptr()
        elif kind == "pinned":
            self.t = torch.from_numpy(np.ascontiguousarray(data).copy()).pin_memory()
            self.ptr = self.t.data_ptr()
        else:
            raw = np.empty(data.size + 64, dtype=np.uint8)
            off = -raw.ctypes.data % 64
            self.a = raw[off:off + data.size]
            self.a[:] = data
            self.ptr = self.a.ctypes.data
        assert self.ptr % 16 == 0

    def read(self):
        import torch
        if self.kind == "device":
            torch.cuda.synchronize()
            return self.t.cpu().numpy()
        return (self.t.numpy() if self.kind == "pinned" else self.a).copy()


class Layout:
    """the two arenas of one call: `inputs[i]` the call's bytes of file i in the engine's layout (may be empty), out_sizes[i] its frames' bytes"""

    def __init__(self, d, kind, inputs, out_sizes, complement):
        self.ain, self.aout = Arena([b.size for b in inputs]), Arena(out_sizes)
        self.fin = fill_bytes(self.ain.total, complement).copy()
        for s, b in zip(self.ain.starts, inputs):
            self.fin[s:s + b.size] = b
        self.fout = fill_bytes(self.aout.total, complement)
        self.min, self.mout = Mem(kind, self.fin), Mem(kind, self.fout)
        self.ios = (d.FileIO * len(inputs))()
        for i, b in enumerate(inputs):
            self.ios[i].dsd = self.min.ptr + self.ain.starts[i]            # (a call of 0 bytes points at its place all the same)
            self.ios[i].pcm = self.mout.ptr + self.aout.starts[i]
            self.ios[i].pcm_capacity_bytes = out_sizes[i]

    def check(self, want, fb, what):
        """every output byte outside the ranges is the fill, inside them `want`; the input arena is as it was"""
        self.got = self.mout.read()
        v = violations(self.aout, self.got, self.fout, want)
        assert not v, f"{what}: {describe(v, fb)}"
        assert np.array_equal(self.min.read(), self.fin), f"{what}: the input arena changed"
        return [self.got[self.aout.starts[i]:self.aout.end(i)] for i in range(len(want))]


class Run:
    """one engine of n files next to one oracle per file; every call through an arena pair"""

    def __init__(self, d, O, kw, n_files, seed, complement, kind="device"):
        assert (d.DBG_NO_COOP, d.DBG_HOST_STAGED) == (DBG_NO_COOP, DBG_HOST_STAGED)
        self.d, self.kw, self.n, self.complement, self.kind = d, dict(kw, filter="E", seed=seed), n_files, complement, kind
        self.e = d.Engine(n_files=n_files, **self.kw)
        okw = {k: v for k, v in self.kw.items() if k not in ENGINE_ONLY + SUBSET}
        self.o = [O.Oracle(**okw) for _ in range(n_files)]
        self.Cin, self.c0, self.C = kw["channels"], kw.get("channel_first", 0), self.e.out_channels
        self.fb = self.e.frame_bytes
        self.sb = self.fb // self.C
        assert self.o[0].frame_bytes == self.sb * self.Cin
        self.peaks = [[0.0] * self.C for _ in range(n_files)]
        self.pos = [0] * n_files
        self.frames = [0] * n_files
        self.names = []

    def pack(self, chans):
        return pack_layout(chans, self.kw["fmt"], self.kw["block_size"]) if chans[0].size else np.zeros(0, dtype=np.uint8)

    def expect(self, inputs):
        """the oracle's frames of the call, the engine's columns of them; the peaks move on"""
        want, nfr = [], []
        for f, buf in enumerate(inputs):
            if not buf.size:
                want.append(None); nfr.append(0)
                continue
            w, fr, y = self.o[f].translate(buf, want_f64=True)
            w = w[:fr * self.sb * self.Cin].reshape(fr, self.Cin, self.sb)[:, self.c0:self.c0 + self.C].reshape(-1)
            if fr:
                self.peaks[f] = [max(p, float(np.abs(y[:fr, self.c0 + c]).max())) for c, p in enumerate(self.peaks[f])]
            want.append(w if fr else None); nfr.append(fr)
        return want, nfr

    def lay_out(self, inputs):
        nfr = [self.e.next_frames(b.size // self.Cin, file=f) for f, b in enumerate(inputs)]
        lay = Layout(self.d, self.kind, inputs, [n * self.fb for n in nfr], self.complement)
        for f, b in enumerate(inputs):
            lay.ios[f].bytes_per_channel = b.size // self.Cin
            lay.ios[f].frames_out = 12345                                  # (the call must write it)
        return lay, nfr

    def settle(self, lay, inputs, planned, kernel, what):
        """after a successful call on `lay`: frames, bytes inside and outside the ranges, peaks, positions, the kernel"""
        want, nfr = self.expect(inputs)
        assert [lay.ios[f].frames_out for f in range(self.n)] == nfr == planned, what
        got = lay.check(want, self.fb, what)
        for f, b in enumerate(inputs):
            self.pos[f] += b.size // self.Cin
            self.frames[f] += nfr[f]
            assert self.e.tell(f) == (self.pos[f], self.frames[f]), what
            assert [self.e.peak(c, file=f) for c in range(self.C)] == self.peaks[f], what
        name = self.e.kernel_name()
        self.names.append(name)
        if kernel is not None:
            assert name == kernel, (what, name)
            assert tile_of(name) * self.fb <= GUARD
        return got

    def call(self, chans, kernel, what=""):
        """one d2d_translate_batch_device of chans[f] = file f's channels (equal lengths, 0 allowed); returns the bytes of every file's range"""
        inputs = [self.pack(c) for c in chans]
        lay, planned = self.lay_out(inputs)
        self.e.translate_batch_device(lay.ios)
        return self.settle(lay, inputs, planned, kernel, what)

    def state(self):
        return [(self.e.tell(f), [self.e.peak(c, file=f) for c in range(self.C)]) for f in range(self.n)]

    def close(self):
        self.e.close()
        for o in self.o:
            o.close()


# ---- call lengths, searched with d2d_next_frames on the engine as it stands ----

def find_bytes(e, f, step, ok, ragged_of=0):
    """the smallest length in steps of `step`, up to LIMIT, for which file f's next call yields a frame count that satisfies ok; ragged_of = B:
    no multiple of the planar block B (a short last block)"""
    for L in range(step, LIMIT + 1, step):
        if ragged_of > 1 and L % ragged_of == 0:
            continue
        if ok(e.next_frames(L, file=f)):
            return L
    return None


def whole_tiles(e, f, B, T):
    """file 0's first call: at least four tiles and a whole number of them, so that the last tile is full and its wide stores end on the file's
    last byte.  Whole blocks where a multiple of the block has such a count below LIMIT (every 44.1k-family route), else the smallest length
    of any size (the 48k family: a short last block), else -- no route needs it -- the most whole tiles LIMIT holds."""
    for k in (4, 3, 2, 1):
        for step in (B, 1):
            L = find_bytes(e, f, step, lambda n: n >= k * T and n % T == 0)
            if L:
                return L
    raise AssertionError("not one whole tile below LIMIT")


def tail(e, f, B, T, residue, longer):
    """a ragged tail: planar routes a short last block, interleaved ones any length; the frame count = residue modulo 4, and either between a
    quarter of a tile and a whole one or beyond one (and no whole number of tiles)"""
    ok = (lambda n: n > T and n % T and n % 4 == residue) if longer else (lambda n: T // 4 <= n < T and n % 4 == residue)
    L = find_bytes(e, f, 1, ok, ragged_of=B)
    assert L, (residue, longer)
    return L


def three_files(d, O, kw, kernels, seed, complement):
    """the scheme of the device-batch cases; returns the kernel names seen and the tails' frame counts"""
    if not isinstance(kernels, (list, tuple)):
        kernels = [kernels] * 3
    T = tile_of(kernels[0])
    fmt_planar = kw["fmt"] == "P"
    B = kw["block_size"] if fmt_planar else 1
    blk = B if fmt_planar else NB
    r = Run(d, O, kw, 3, seed, complement)
    e, Cin = r.e, r.Cin
    streams = [[random_bytes(1 << 18, 1000 * seed + 10 * f + c) for c in range(Cin)] for f in range(3)]
    at = [0, 0, 0]

    def take(lens):
        ch = [[s[at[f]:at[f] + n] for s in streams[f]] for f, n in enumerate(lens)]
        for f, n in enumerate(lens):
            at[f] += n
        return ch

    # call 1: whole tiles and whole blocks | a few blocks, no whole number of tiles | one block (where that is under a tile -- every route but
    # M = 8, M = 16 and the one-output-per-lane kernels -- the careful path alone; the short tails below are under a tile on every route)
    L0 = whole_tiles(e, 0, B, T)
    n0 = e.next_frames(L0, file=0)
    assert n0 % T == 0 and n0 >= 4 * T, (L0, n0, T)
    # a few hundred bytes of all-ones and all-zeros inside file 0: both rails, the integer routes' careful / redo tiles (in the first call; where
    # four tiles of 64 outputs are shorter than that, in the second call's blocks)
    s0 = (L0 // 4, L0 // 2) if L0 >= 2400 else (L0 + blk // 4, L0 + blk)
    for c in range(Cin):
        streams[0][c][s0[0]:s0[0] + 300] = 0xFF
        streams[0][c][s0[1]:s0[1] + 300] = 0x00
    # (where every block is a whole number of tiles -- tiles of 512 and of 64 outputs -- the few blocks get a short one behind them)
    L1 = next((k * blk for k in (3, 5, 2, 7) if e.next_frames(k * blk, file=1) % T), None) or \
        next(n for n in range(3 * blk + blk // 2, 4 * blk) if e.next_frames(n, file=1) % T)
    r.call(take([L0, L1, blk]), kernels[0], "call 1")
    # call 2: a few more blocks | 0 bytes | a ragged tail
    t2 = tail(e, 2, B, T, 3, False)
    tails = [e.next_frames(t2, file=2)]
    r.call(take([2 * blk, 0, t2]), kernels[1], "call 2")
    # call 3: a ragged tail | a ragged tail | 0 bytes
    t0, t1 = tail(e, 0, B, T, 1, True), tail(e, 1, B, T, 2, False)
    tails += [e.next_frames(t0, file=0), e.next_frames(t1, file=1)]
    # the partial groups of a lane's four frames, a tail under a tile and one over
    assert sorted(n % 4 for n in tails) == [1, 2, 3] and min(tails) < T < max(tails), tails
    r.call(take([t0, t1, 0]), kernels[2], "call 3")
    r.close()
    return r.names, tails


# ---- the routes ----

EXTRA = {
    # five channels planar: two pairs and a single channel left over on the two-group kernel, each group storing its part of the 15-byte frames
    "five_channels_t24": (dict(dsd_rate=1, output_rate=88200, channels=5, bit_depth=24, dither="T", **PL), "d2d_fir_mfma2_kernel<4, 13, 2, 0>"),
    # a channel subset of three out of six
    "six_channels_1_to_3_r16": (dict(dsd_rate=1, output_rate=88200, channels=6, channel_first=1, channel_count=3, bit_depth=16, dither="R", **PL), "d2d_fir_mfma2_kernel<4, 13, 2, 0>"),
    "six_channels_1_to_3_t20": (dict(dsd_rate=1, output_rate=88200, channels=6, channel_first=1, channel_count=3, bit_depth=20, dither="T", **PL), "d2d_fir_mfma2_kernel<4, 13, 2, 0>"),
    # the cascade with three channels: stage B stores a pair inside a 9-byte frame plus a single; with eight at 16-bit
    "cascade_3ch_dsd256_96k": (dict(dsd_rate=4, output_rate=96000, channels=3, bit_depth=24, dither="T", **PL), "d2d_fir_mfma2_kernel<4, 10, 2, 2>"),
    "cascade_8ch_s16": (dict(dsd_rate=4, output_rate=96000, channels=8, bit_depth=16, dither="T", **PL), "d2d_fir_mx_kernel<4, 352, 3, 0, 0, 1, 5>"),
    # 32-bit taps through the two scratch passes: the combining pass writes the frames
    "taps32_two_pass": (dict(dsd_rate=1, output_rate=88200, channels=2, bit_depth=24, dither="T", tap_bits=32, debug=DBG_TAPS32_2PASS, **PL), TWO_PASS_KERNEL),
    # byte-interleaved stereo through the planar pre-pass
    "fp6_il2_no_coop": (dict(ROUTES["fp6_il2"][0], debug=DBG_NO_COOP), ROUTES["fp6_il2"][1]),
    # the noise shaper's f64 loop and its general kernel on stereo (they run behind the FIR kernel named here)
    "ns_s16_no_intq": (dict(NS_ROUTES["ns_s16_0db"][0], debug=DBG_NO_INTQ), NS_ROUTES["ns_s16_0db"][1]),
    "ns_s24_general": (dict(NS_ROUTES["ns_s24_m2db"][0], debug=DBG_NS_GENERAL), NS_ROUTES["ns_s24_m2db"][1]),
    # a mono engine: the first call's files all split into halves (the pair), the calls with a ragged or an empty file take the ordinary mono kernel
    "mono_ragged": (MONO, [PAIR_KERNEL, MONO_KERNEL, MONO_KERNEL]),
}
ALL_ROUTES = dict(ROUTES, **NS_ROUTES, **EXTRA)
assert len(ALL_ROUTES) == len(ROUTES) + len(NS_ROUTES) + len(EXTRA)
DEVICE_CASES = sorted(ROUTES) + sorted(NS_ROUTES) + list(EXTRA)


@gpu
@pytest.mark.parametrize("route", DEVICE_CASES)
def test_device_batch_stays_inside_its_frames(engine_lib, oracle_mod, route):
    kw, kernels = ALL_ROUTES[route]
    seed = 4000 + DEVICE_CASES.index(route)
    seen = []
    for complement in (False, True):
        names, tails = three_files(engine_lib, oracle_mod, kw, kernels, seed, complement)
        seen.append((names, tails))
    assert seen[0] == seen[1]
    print("kernels:", route, seen[0][0])


# ---- the mono pair ----

M128_PAIR = dict(MONO, dsd_rate=4, block_size=4112, kernel=2)      # 16 bytes per output: a block of 16 * 257 bytes holds an odd number of frames
PAIRS = {
    "t24": (MONO, PAIR_KERNEL),
    "r16": (dict(MONO, bit_depth=16, dither="R"), "d2d_fir_mx_kernel<4, 560, 3, 2, 2, 1, 5>"),
    "f32": (dict(MONO, bit_depth=32, dither="F"), "d2d_fir_mx_kernel<4, 560, 3, 7, 4, 1, 5>"),
    "b4112_t24": (dict(MONO, block_size=4112), PAIR_KERNEL),
    "m64_t24": (dict(MONO, dsd_rate=2, block_size=4112), "d2d_fir_mx_kernel<8, 1104, 2, 1, 3, 1, 5>"),
    "m128_odd_t24": (M128_PAIR, ROUTES["fp6_m128_t24"][1]),
    "m128_odd_r16": (dict(M128_PAIR, bit_depth=16, dither="R"), "d2d_fir_mx_kernel<16, 2192, 1, 2, 2, 1, 5>"),
}


@gpu
@pytest.mark.parametrize("case", list(PAIRS))
def test_mono_pair_second_half_starts_where_the_first_ends(engine_lib, oracle_mod, case):
    """two files, every call two equal halves of an odd number of whole blocks.  M = 128: the first half's frame count is odd and the second
    half starts at a byte that is no multiple of 4; M = 64 with blocks of 4112 bytes: an even count that is no multiple of 4, the second half
    at 2 modulo 4; M = 32: a multiple of four frames (the pair's own condition: see the module's text), with blocks of 4112 bytes the second
    half 12 bytes off a multiple of 16"""
    kw, kernel = PAIRS[case]
    B, seed = kw["block_size"], 4100 + list(PAIRS).index(case)
    seen = []
    for complement in (False, True):
        r = Run(engine_lib, oracle_mod, kw, 2, seed, complement)
        streams = [random_bytes(1 << 18, 1000 * seed + f) for f in range(2)]
        streams[0][3000:3300] = 0xFF
        streams[0][9000:9300] = 0x00
        at = [0, 0]
        for call, halves in enumerate([(3, 1), (1, 5), (5, 3)]):
            lens = [2 * k * B for k in halves]
            first = [r.e.next_frames(n, file=f) // 2 for f, n in enumerate(lens)]
            if kw["dsd_rate"] == 4:
                assert all(n % 2 == 1 and (n * r.fb) % 4 for n in first), first
            elif kw["dsd_rate"] == 2:
                assert all(n % 4 == 2 and (n * r.fb) % 4 == 2 for n in first), first
            else:
                assert all(n % 4 == 0 and ((n * r.fb) % 16 != 0) == (B == 4112) for n in first), first
            r.call([[streams[f][at[f]:at[f] + n]] for f, n in enumerate(lens)], kernel, f"call {call + 1}")
            at = [a + n for a, n in zip(at, lens)]
        r.close()
        seen.append(r.names)
    assert seen[0] == seen[1]
    print("kernels:", "mono_pair_" + case, seen[0])


# ---- one long case per pipelined family ----

@gpu
@pytest.mark.parametrize("route", ["fp6_m32_t24", "int8_m8_t24", "px_kind1_dsd64_96k", "fp6_six_channels"])
def test_long_stream_whose_waves_walk_several_tiles(engine_lib, oracle_mod, route):
    """a single file sized like test_f64_flavour_when_waves_walk_several_tiles (tests/test_gpu_parity.py): the fixed-order loop's first trip
    stores a tile early and rewrites it.  The length ends on a full tile; both fills; the oracle's frames are computed once for the two runs"""
    kw, kernel = ROUTES[route]
    T, seed = tile_of(kernel), 4200
    M = 2822400 * kw["dsd_rate"] // kw["output_rate"]
    nbytes = 6_000_000 * (4 if M >= 32 else 1)
    B = kw["block_size"]
    chans, ref = None, None
    for complement in (False, True):
        r = Run(engine_lib, oracle_mod, kw, 1, seed, complement)
        if chans is None:
            first = -(-nbytes // B) * B
            # whole blocks if some multiple of the block ends on a tile soon, else (the 48k family) a short last block
            L = next((n for n in range(first, first + 600 * B, B) if r.e.next_frames(n) % T == 0), None) or \
                next(n for n in range(first, first + (1 << 16)) if r.e.next_frames(n) % T == 0)
            chans = [random_bytes(L, 100 * seed + c) for c in range(r.Cin)]
            buf = r.pack(chans)
        assert r.e.next_frames(L) % T == 0 and r.e.next_frames(L) > 2048 * 3 * T // 2
        lay, planned = r.lay_out([buf])
        r.e.translate_batch_device(lay.ios)
        if ref is None:
            ref = r.expect([buf])
            ref_peaks = r.peaks
        r.expect = lambda inputs: ref                        # (the same stream, the same parameters: the second run shares the first one's reference)
        r.peaks = ref_peaks
        r.settle(lay, [buf], planned, kernel, route)
        r.close()
    print("kernels:", route, r.names)


# ---- host entry points: the same kernels; what differs is the memory and the copies ----

HOST_ROUTES = {k: ALL_ROUTES[k] for k in ("fp6_m32_t24", "px_kind1_dsd64_96k", "cascade_dsd256_96k", "ns_s16_0db")}
HOST_MODES = {"pinned_direct": ("pinned", 0), "pinned_staged": ("pinned", DBG_HOST_STAGED), "pageable": ("pageable", 0)}


def host_run(d, O, kw, n_files, seed, complement, mode):
    kind, flag = HOST_MODES[mode]
    return Run(d, O, dict(kw, debug=kw.get("debug", 0) | flag), n_files, seed, complement, kind=kind)


@gpu
@pytest.mark.parametrize("route", list(HOST_ROUTES))
def test_translate_on_host_arenas(engine_lib, oracle_mod, route):
    """d2d_translate with exact capacity on a pinned arena (the kernels store across the link), the same staged, and on pageable memory (the
    staged download's size): five calls each -- whole tiles, two blocks, three ragged tails -- and the three ways give the same bytes"""
    kw, kernel = HOST_ROUTES[route]
    T, B, seed = tile_of(kernel), kw["block_size"], 4300 + list(HOST_ROUTES).index(route)
    outs = {}
    for complement in (False, True):
        for mode in HOST_MODES:
            r = host_run(engine_lib, oracle_mod, kw, 1, seed, complement, mode)
            streams = [random_bytes(1 << 18, 1000 * seed + c) for c in range(r.Cin)]
            at, got = 0, []
            for call in range(5):
                L = [lambda: whole_tiles(r.e, 0, B, T), lambda: 2 * B, lambda: tail(r.e, 0, B, T, 1, True), lambda: tail(r.e, 0, B, T, 2, False),
                     lambda: tail(r.e, 0, B, T, 3, False)][call]()
                inputs = [r.pack([s[at:at + L] for s in streams])]
                at += L
                lay, planned = r.lay_out(inputs)
                io = lay.ios[0]
                io.frames_out = r.e.translate_into(io.dsd, io.bytes_per_channel, io.pcm, io.pcm_capacity_bytes)
                got += r.settle(lay, inputs, planned, kernel, f"{mode}, call {call + 1}")
            outs[mode, complement] = np.concatenate(got)
            r.close()
    assert all(np.array_equal(o, outs["pinned_direct", False]) for o in outs.values())
    print("kernels:", route, sorted(set(r.names)))


@gpu
@pytest.mark.parametrize("mode", list(HOST_MODES))
@pytest.mark.parametrize("route", list(HOST_ROUTES))
def test_batch_host_on_host_arenas(engine_lib, oracle_mod, route, mode):
    """d2d_translate_batch_host, three ragged files, 8192-byte slices where the pipeline runs; a second call with an empty file carries the state"""
    kw, kernel = HOST_ROUTES[route]
    B, seed = kw["block_size"], 4400 + list(HOST_ROUTES).index(route)
    for complement in (False, True):
        r = host_run(engine_lib, oracle_mod, kw, 3, seed, complement, mode)
        streams = [[random_bytes(1 << 17, 1000 * seed + 10 * f + c) for c in range(r.Cin)] for f in range(3)]
        at = [0, 0, 0]
        for call, lens in enumerate([[B * 7 + 123, B * 3, B * 12 + 4000], [B * 2 + 1, 0, 777]]):
            inputs = [r.pack([s[at[f]:at[f] + n] for s in streams[f]]) for f, n in enumerate(lens)]
            at = [a + n for a, n in zip(at, lens)]
            lay, planned = r.lay_out(inputs)
            r.e.translate_batch_host(lay.ios, 8192)
            r.settle(lay, inputs, planned, kernel, f"{mode}, call {call + 1}")
        r.close()


@gpu
@pytest.mark.parametrize("route", list(HOST_ROUTES))
def test_convert_stream_hands_whole_frames_to_the_sink(engine_lib, oracle_mod, route):
    """d2d_convert_stream: every write callback receives whole frames, their byte counts add up to the oracle's, and the bytes are the oracle's"""
    kw, kernel = HOST_ROUTES[route]
    kw = dict(kw, filter="E", seed=4500)
    B, C_ = kw["block_size"], kw["channels"]
    nbytes = B * 10 + 1234
    chans = [random_bytes(nbytes, 4500 + c) for c in range(C_)]
    pos = [0]

    def read(cap):
        assert cap % B == 0
        a = pos[0]
        b = min(nbytes, a + min(cap, 3 * B))
        pos[0] = b
        return pack_layout([c[a:b] for c in chans], "P", B).tobytes() if b > a else b""

    writes = []
    e = engine_lib.Engine(**kw)
    e.convert_stream(read, writes.append, total_bytes_per_channel=nbytes, chunk_bytes_per_channel=3 * B)
    o = oracle_mod.Oracle(**{k: v for k, v in kw.items() if k not in ENGINE_ONLY})
    w, fr = o.translate(pack_layout(chans, "P", B))
    fb = e.frame_bytes
    assert len(writes) == 4 and all(len(x) > 0 and len(x) % fb == 0 for x in writes), [len(x) for x in writes]
    assert sum(len(x) for x in writes) == fr * fb
    assert np.array_equal(np.frombuffer(b"".join(writes), dtype=np.uint8), w[:fr * fb])
    assert e.kernel_name() == kernel and e.tell() == (nbytes, fr)
    e.close()
    o.close()


# ---- prime writes nothing ----

@gpu
@pytest.mark.parametrize("route", ["cascade_dsd256_96k", "fp6_m32_t24", "ns_s16_0db"])
def test_prime_writes_no_pcm(engine_lib, oracle_mod, route):
    """d2d_prime_batch_device with pcm pointing into a filled arena and a capacity that is not 0: the arena stays as it is, frames_out = 0, the
    positions move on (stage A of the cascade runs); the translate behind it equals the oracle's continuation and stays inside its range"""
    kw, kernel = ALL_ROUTES[route]
    B, seed = kw["block_size"], 4600
    for complement in (False, True):
        r = Run(engine_lib, oracle_mod, kw, 2, seed, complement)
        align = r.e.slice_align_bytes()                   # (the noise shaper starts on a segment boundary only)
        lens = [align, align] if align > 1 else [B + 777, 2 * B]
        streams = [[random_bytes(1 << 17, 1000 * seed + 10 * f + c) for c in range(r.Cin)] for f in range(2)]
        inputs = [r.pack([s[:n] for s in streams[f]]) for f, n in enumerate(lens)]
        lay = Layout(engine_lib, "device", inputs, [4096, 1000 * r.fb], complement)
        for f, n in enumerate(lens):
            lay.ios[f].bytes_per_channel = n
            lay.ios[f].frames_out = 12345
        r.e.prime_batch_device(lay.ios)
        lay.check([None, None], r.fb, "prime")
        for f, n in enumerate(lens):
            _, fr = r.o[f].translate(inputs[f])           # the oracle converts the same bytes; their frames are not the slice's
            assert fr > 0 and lay.ios[f].frames_out == 0
            r.pos[f], r.frames[f] = n, fr
            assert r.e.tell(f) == (n, fr)
        assert r.state() == [((n, r.frames[f]), [0.0] * r.C) for f, n in enumerate(lens)]
        nxt = [3 * B + 555, B]
        r.call([[s[n:n + m] for s in streams[f]] for f, (n, m) in enumerate(zip(lens, nxt))], kernel, "the translate behind the prime")
        r.close()


# ---- failed calls change nothing ----

def refused(r, lay, call, code, text):
    """`call` fails with `code`; no byte of either arena, no position and no peak has changed"""
    L = r.d.lib()
    before = r.state()
    assert call() == code, L.d2d_last_error(r.e._h)
    assert text in L.d2d_last_error(r.e._h)
    lay.check([None] * r.n, r.fb, f"a call refused with {code}")
    assert r.state() == before


@gpu
@pytest.mark.parametrize("route", ["fp6_m32_t24", "px_kind1_dsd64_96k", "cascade_dsd256_96k"])
def test_refused_device_batch_changes_nothing(engine_lib, oracle_mod, route):
    """three files that have state; file 2's buffer one byte short: D2D_ERR_CAPACITY, a misaligned pcm: D2D_ERR_PARAM.  Every byte, every
    frames_out (plan_call's promise), tell and peak stay; the same call with the right arguments then gives the oracle's bytes"""
    kw, kernel = ALL_ROUTES[route]
    B, seed = kw["block_size"], 4700
    L = engine_lib.lib()
    for complement in (False, True):
        r = Run(engine_lib, oracle_mod, kw, 3, seed, complement)
        streams = [[random_bytes(1 << 17, 1000 * seed + 10 * f + c) for c in range(r.Cin)] for f in range(3)]
        first, then = [2 * B, 3 * B, B], [B + 333, 2 * B, 3 * B + 17]
        r.call([[s[:n] for s in streams[f]] for f, n in enumerate(first)], kernel, "the first call")
        inputs = [r.pack([s[a:a + n] for s in streams[f]]) for f, (a, n) in enumerate(zip(first, then))]
        lay, planned = r.lay_out(inputs)
        call = lambda: L.d2d_translate_batch_device(r.e._h, lay.ios, 3, None)
        lay.ios[2].pcm_capacity_bytes -= 1
        refused(r, lay, call, -20, b"too small")
        lay.ios[2].pcm_capacity_bytes += 1
        lay.ios[1].pcm += 4
        refused(r, lay, call, -1, b"aligned")
        lay.ios[1].pcm -= 4
        assert [lay.ios[f].frames_out for f in range(3)] == [12345] * 3
        r.e.translate_batch_device(lay.ios)
        r.settle(lay, inputs, planned, kernel, "the call behind the refused ones")
        r.close()


@gpu
@pytest.mark.parametrize("mode", list(HOST_MODES))
@pytest.mark.parametrize("route", ["fp6_m32_t24", "cascade_dsd256_96k"])
def test_refused_host_batch_changes_nothing(engine_lib, oracle_mod, route, mode):
    """d2d_translate_batch_host with 8192-byte slices; file 1's buffer is one FRAME short of its total, which only its last slice would overflow:
    the pinned path fails in its plan; the pipeline used to fail at that slice's download, with the earlier slices in the caller's buffers and the
    files moved on.  All three ways now refuse the call before anything is staged"""
    kw, kernel = ALL_ROUTES[route]
    B, seed = kw["block_size"], 4800
    L = engine_lib.lib()
    for complement in (False, True):
        r = host_run(engine_lib, oracle_mod, kw, 3, seed, complement, mode)
        streams = [[random_bytes(1 << 17, 1000 * seed + 10 * f + c) for c in range(r.Cin)] for f in range(3)]
        first, then = [2 * B, 3 * B, B], [3 * B, 7 * B + 123, 2 * B]
        inputs = [r.pack([s[:n] for s in streams[f]]) for f, n in enumerate(first)]
        lay, planned = r.lay_out(inputs)
        r.e.translate_batch_host(lay.ios, 8192)
        r.settle(lay, inputs, planned, kernel, "the first call")
        inputs = [r.pack([s[a:a + n] for s in streams[f]]) for f, (a, n) in enumerate(zip(first, then))]
        lay, planned = r.lay_out(inputs)
        call = lambda: L.d2d_translate_batch_host(r.e._h, lay.ios, 3, 8192)
        assert then[1] > 3 * 8192 and planned[1] > 1
        lay.ios[1].pcm_capacity_bytes -= r.fb
        refused(r, lay, call, -20, b"too small")
        lay.ios[1].pcm_capacity_bytes += r.fb
        pcm2, lay.ios[2].pcm = lay.ios[2].pcm, None
        refused(r, lay, call, -1, b"pcm")
        lay.ios[2].pcm = pcm2
        r.e.translate_batch_host(lay.ios, 8192)
        r.settle(lay, inputs, planned, kernel, "the call behind the refused ones")
        r.close()
