"""The inputs of tests/test_gpu_flac_search_edges.py -- flac_search_kernel<CH, LPC>, FLAC efforts 1 and 12 on the GPU -- and the proof
that they are what that file needs them to be.  No GPU.

  1. The edge corpora of tests/test_flac_edges_cpu.py (K_SWEEP, K_EDGES, SPIKES, SHORT_FILES, MANY_BLOCKS) at efforts 1 and 12: the
     host encoder (d2d_flac_encode_host_effort, the GPU tests' reference) equals the Python restatements (flac_search_ref,
     flac_lpc_ref) and decodes back to the input through d2d_flac_decode_host.
  2. EDGE_CASES, a corpus that attains the integer bounds dsd2dxd_amd/csrc/flac/d2d_flac.hip states for the search kernel and fires
     the branches of rule 13 (flac_lpc.h, lpc_coefficients) that audio-like signals do not reach; test_the_cases_reach_the_kernels_bounds
     proves from the restatement what every signal is there for and pins what the corpus attains.
  3. d2d_flac_verify_host_method at both methods on what the host encoder makes of EDGE_CASES, and on one flipped PCM bit.
  4. VECTORS: hand-made and seeded autocorrelations for the routine itself, tools/flac_lpc_probe.cpp built with g++ against the
     restatement; tools/flac_lpc_probe_gpu.hip runs the same list on the device in the GPU file."""
import functools
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import flac_lpc_ref as P
import flac_ref as R
import flac_search_ref as S
import test_flac_edges_cpu as E
from test_flac_lpc_cpu import HAND, from_reflection
from test_flac_verify_cpu import BAD_SAMPLES, clean, frame_sizes, nblocks

B = R.BLOCK
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EFFORTS = (1, 12)
RESTATED = {1: S.encode, 12: P.encode}


# ---- 1. the effort-0 edge corpora at efforts 1 and 12 -------------------------------------------------------------------------------

def unpacked(back, channels, depth):
    return R.unpack_pcm(np.frombuffer(back, dtype=np.uint8), channels, depth)


def check_host(d, samples, depth, effort, first_block=0, final=True, restated=True):
    """the host encoder at `effort`: its record, frames consumed, every frame within the bound, the round trip through
    d2d_flac_decode_host; with `restated` the bytes are the Python restatement's.  Returns the frame sizes."""
    samples = np.asarray(samples, dtype=np.int64)
    frames, ch = samples.shape
    got, res, consumed = d.flac_encode_host(ch, depth, R.pack_pcm(samples, depth), first_block=first_block, final=final, effort=effort)
    assert consumed == (frames if final else frames // B * B)
    blocks = nblocks(consumed)
    if restated:
        want, sizes, used = RESTATED[effort](samples, depth, first_block=first_block, final=final)[:3]
        assert got == want
        assert (res.bytes_out, res.min_frame_bytes, res.max_frame_bytes, consumed) == (sum(sizes), min(sizes, default=0), max(sizes, default=0), used)
    back, frames_out, chk = d.flac_decode_host(ch, depth, got, first_block=first_block)
    assert frames_out == consumed and chk.as_tuple() == clean(consumed, blocks), chk.as_tuple()
    assert np.array_equal(unpacked(back, ch, depth)[:consumed], samples[:consumed])
    if not restated:                                               # the sizes: frames are independent, each block by itself is its frame
        sizes = [len(d.flac_encode_host(ch, depth, R.pack_pcm(samples[a:a + B], depth), first_block=first_block + i, effort=effort)[0])
                 for i, a in enumerate(range(0, consumed, B))]
        assert (res.bytes_out, res.min_frame_bytes, res.max_frame_bytes) == (sum(sizes), min(sizes, default=0), max(sizes, default=0))
    for i, fs in enumerate(sizes):
        assert fs <= R.frame_bound(ch, depth, min(B, frames - B * i)), i
    return sizes


@pytest.mark.parametrize("effort", EFFORTS)
@pytest.mark.parametrize("depth", E.DEPTHS)
def test_k_sweep(engine_lib, depth, effort):
    for d, kind, a in E.K_SWEEP:
        if d == depth:
            check_host(engine_lib, E.k_sweep_signal(d, kind, a), d, effort)


@pytest.mark.parametrize("effort", EFFORTS)
def test_k_edges(engine_lib, effort):
    for n, d, j in E.K_EDGES:
        check_host(engine_lib, E.k_edge_signal(n, d, j), d, effort)


# one spike of each position against the restatements (amplitude and floor by turns), every one against the decoder
SPIKE_KINDS = ((16, "full", 0), (24, 40, 1), (24, "full", 1), (16, 40, 0))                  # (depth, amplitude, floor)
SPIKE_RESTATED = {at: (SPIKE_KINDS[k % 4][0],) + at + SPIKE_KINDS[k % 4][1:] for k, at in enumerate(E.SPIKE_AT)}


@pytest.mark.parametrize("effort", EFFORTS)
def test_spikes(engine_lib, effort):
    assert set(SPIKE_RESTATED) == set(E.SPIKE_AT) and set(SPIKE_RESTATED.values()) <= set(E.SPIKES)
    for spec in E.SPIKES:
        d, frames, i, amp, floor = spec
        check_host(engine_lib, E.spike_signal(*spec), d, effort, restated=SPIKE_RESTATED[(frames, i)] == spec)


# every SHORT_N alone against the restatements, each at one of the shapes; every file of every shape against the decoder
@pytest.mark.parametrize("effort", EFFORTS)
@pytest.mark.parametrize("channels,depth", E.SHORT_SHAPES)
def test_short_last_blocks(engine_lib, channels, depth, effort):
    mine = [n for k, n in enumerate(E.SHORT_N) if E.SHORT_SHAPES[k % len(E.SHORT_SHAPES)] == (channels, depth)]
    assert mine
    for lead, n in E.SHORT_FILES:
        check_host(engine_lib, E.short_signal(channels, depth, lead, n), depth, effort, first_block=3, restated=lead == 0 and n in mine)


@pytest.mark.parametrize("effort", EFFORTS)
@pytest.mark.parametrize("spec", E.MANY_BLOCKS, ids=lambda s: f"{s[0]}ch{s[1]}-{s[2]}x4096+{s[3]}")
def test_many_blocks_round_trip(engine_lib, spec, effort):
    """files of up to 300 blocks: against the decoder alone (the restatements take a tenth of a second per block)"""
    x = E.many_blocks_signal(spec)
    ch, depth = spec[:2]
    got, res, consumed = engine_lib.flac_encode_host(ch, depth, R.pack_pcm(x, depth), first_block=spec[4], final=spec[5], effort=effort)
    back, frames_out, chk = engine_lib.flac_decode_host(ch, depth, got, first_block=spec[4])
    assert frames_out == consumed and chk.as_tuple() == clean(consumed, E.many_blocks_count(spec))
    assert np.array_equal(unpacked(back, ch, depth)[:consumed], x[:consumed])
    assert res.bytes_out == len(got) <= R.bound_bytes(ch, depth, x.shape[0], spec[5])


# ---- 2. EDGE_CASES -----------------------------------------------------------------------------------------------------------------------
# Rail signals: every sample is the largest or the smallest value of its depth.

SHAPES = tuple((ch, d) for ch in (1, 2, 3, 8) for d in (16, 20, 24))
SHORTS = (64, 65, 67, 1000, 259, 130)                              # the short block behind a family's whole one; 65, 67, 259: n % 4 != 0
FIRSTS = (0x7F, 0x7FF, 0xFFFF, 0x1FFFFF, 0x3FFFFFF, 0, 5)          # the second frame's number takes a byte more than the first's
PERIODS = tuple(range(2, 26))
SIDE_MAX = (1 << 24) - 1                                            # |L - R| of anti-phase rails at depth 24
FIXED_MAX = 16 * SIDE_MAX                                           # ... and its order-4 difference: 2^28 - 16


def rails(depth):
    return (1 << (depth - 1)) - 1, -(1 << (depth - 1))


def antiphase(n, depth):
    """L = +/- max by turns, R = -1 - L: the side signal is +/- (2^depth - 1), alternating"""
    top, bot = rails(depth)
    left = np.where(np.arange(n) % 2 == 0, top, bot).astype(np.int64)
    return np.stack([left, -1 - left], axis=1)


def random_rails(n, ch, depth, seed):
    top, bot = rails(depth)
    return np.where(np.random.default_rng(seed).integers(0, 2, size=(n, ch)) == 1, top, bot).astype(np.int64)


def squares(n, depth, periods):
    """one full-scale square per channel, of the period given, each at a phase of its own"""
    top, bot = rails(depth)
    i = np.arange(n)
    return np.stack([np.where((i + 3 * c) % per < per // 2, top, bot) for c, per in enumerate(periods)], axis=1).astype(np.int64)


def dc(n, ch, depth, flip):
    top, bot = rails(depth)
    return np.stack([np.full(n, top if (c + flip) % 2 == 0 else bot) for c in range(ch)], axis=1).astype(np.int64)


def impulses(lengths, depth, at):
    """silence with full-scale impulses (+, -, ...) at the places `at(n)` of every block of `lengths`, one channel"""
    top, bot = rails(depth)
    blocks = []
    for n in lengths:
        x = np.zeros((n, 1), dtype=np.int64)
        for k, i in enumerate(at(n)):
            x[i, 0] = bot if k % 2 else top
        blocks.append(x)
    return np.concatenate(blocks)


def poles(ks, n, depth, seed):
    """white noise through the all-pole filter whose reflection coefficients are ks, scaled to 0.9 of full scale"""
    a = [1.0]
    for m, k in enumerate(ks, 1):
        new = a + [0.0]
        for j in range(1, m):
            new[j] = a[j] - k * a[m - j]
        new[m] = k
        a = new
    a = a[1:]
    m, lead = len(a), 2000
    e = [float(v) for v in np.random.default_rng(seed).standard_normal(n + lead)]
    y = [0.0] * m
    for v in e:                                                    # Python floats, added in the order written: the same samples everywhere
        for j in range(m):
            v = v + a[j] * y[-1 - j]
        y.append(v)
    y = np.array(y[lead + m:])
    return np.rint(y / np.abs(y).max() * 0.9 * rails(depth)[0]).astype(np.int64).reshape(-1, 1)


def near_rails(n, depth, seed, swap):
    """a full-scale square and the same a few steps inside the rails: the difference is small noise, so that a side subframe pays
    beside a rail-level LPC one; `swap` puts the noisier channel first"""
    top, bot = rails(depth)
    a = squares(n, depth, (13,))[:, 0]
    e = np.random.default_rng(seed).integers(0, 40, size=n)
    b = np.where(a > 0, a - e, a + e)
    return np.stack([b, a] if swap else [a, b], axis=1).astype(np.int64)


def _case(name, samples, depth, first_block=0, final=True):
    return dict(name=name, samples=np.asarray(samples, dtype=np.int64), depth=depth, first_block=first_block, final=final)


def _build_cases():
    cases = []
    # anti-phase rails: a whole block and a short one, the shortest LPC frames, n % 4 != 0, a file that is not final
    cases.append(_case("antiphase", antiphase(B + 1000, 24), 24, 0x7F))
    cases += [_case("antiphase-%d" % n, antiphase(n, 24), 24, 0x800 + n) for n in (64, 65, 67)]
    cases.append(_case("antiphase-not-final", antiphase(B + 500, 24), 24, 0x7FF, False))
    # random rails, squares of every period from 2 to 25, DC of both signs: every (channels, depth), a whole block and a short one
    period = 0
    for i, (ch, d) in enumerate(SHAPES):
        cases.append(_case("rails-%dch%d" % (ch, d), random_rails(B + SHORTS[i % 6], ch, d, i), d, FIRSTS[i % 7]))
        pers = [PERIODS[(period + c) % len(PERIODS)] for c in range(ch)]
        period += ch
        cases.append(_case("squares-%dch%d" % (ch, d), squares(B + SHORTS[(i + 1) % 6], d, pers), d, FIRSTS[(i + 2) % 7]))
        cases.append(_case("dc-%dch%d" % (ch, d), dc(B + SHORTS[(i + 2) % 6], ch, d, i), d, FIRSTS[(i + 4) % 7]))
    # the other stereo assignments with a rail-level LPC subframe
    cases += [_case("near-rails-%d" % swap, near_rails(B + 67, 24, 50 + swap, swap), 24) for swap in (0, 1)]
    cases.append(_case("two-squares", squares(B + 64, 16, (13, 17)), 16))
    # impulses: one (R(l) == 0 for l > 0: cmax == 0, no candidate), two fewer than twelve samples apart (order 4, or 4 and 8, dropped)
    lengths = (B, 1000)
    cases.append(_case("impulse-first", impulses(lengths, 24, lambda n: (0,)), 24))
    cases.append(_case("impulse-middle", impulses(lengths, 16, lambda n: (n // 2,)), 16))
    cases.append(_case("impulses-5-apart", impulses(lengths, 24, lambda n: (n // 2, n // 2 + 5)), 24))
    cases.append(_case("impulses-11-apart", impulses(lengths, 20, lambda n: (n // 2, n // 2 + 11)), 20))
    # all twelve reflection coefficients at +/- 0.9: orders 8 and 12 are dropped at sum |q| > 62 * 2^shift; shorter blocks keep them, at
    # shifts of 8 and 9; tiny noise has the shift clamped at 15
    cases += [_case("poles%+.1f" % k, poles([k] * 12, B, 24, 3), 24) for k in (0.9, -0.9)]
    cases += [_case("poles%+.1f-1000" % k, poles([k] * 12, 1000, 24, 3), 24) for k in (0.9, -0.9)]
    cases.append(_case("poles-by-turns-64", poles([0.9, -0.9] * 6, 64, 24, 3), 24))
    cases.append(_case("tiny", np.random.default_rng(4).integers(-4, 5, size=(1000, 1)), 16))
    return cases


EDGE_CASES = _build_cases()
EDGE_IDS = [c["name"] for c in EDGE_CASES]
EDGE_GROUPS = sorted({(c["samples"].shape[1], c["depth"]) for c in EDGE_CASES})


@functools.lru_cache(maxsize=None)
def restated(i):
    """(bytes, sizes, consumed, infos) of EDGE_CASES[i] at effort 12 by the restatement: computed once (its plan() asserts |r| < 2^30 for
    every LPC residual set it computes)"""
    c = EDGE_CASES[i]
    return P.encode(c["samples"], c["depth"], first_block=c["first_block"], final=c["final"])


def fixed_sets(x):
    """the five residual sets the kernel computes for a signal: orders 0 .. 4"""
    rs = [x]
    for _ in range(4):
        rs.append(rs[-1][1:] - rs[-1][:-1])
    return rs


def lpc_sets(x):
    """{P: the residual set of every candidate that exists}, and the autocorrelation"""
    r13 = P.autocorrelation(x)
    return {m: P.residuals(x, q, sh) for m, (q, sh) in P.coefficients(r13)[0].items()}, r13


def reached(r13):
    """[(m, max |a[j]|)] for the orders 4, 8, 12 that rule 13's recursion reaches on R: flac_lpc_ref.coefficients' own arithmetic, to
    tell a candidate dropped at |a| >= 2^13 from one dropped at sum |q| > 62 * 2^shift"""
    out = []
    if r13[0] == 0:
        return out
    a, err = [0.0] * 13, float(r13[0])
    for m in range(1, 13):
        acc = float(r13[m])
        for j in range(1, m):
            acc = acc - a[j] * float(r13[m - j])
        k = acc / err
        a = [a[0]] + [a[j] - k * a[m - j] for j in range(1, m)] + [k] + a[m + 1:]
        err = err * (1.0 - k * k)
        if not err > 0:
            break
        if m in P.ORDERS:
            out.append((m, max(abs(v) for v in a[1:m + 1])))
    return out


def _k(r, n, order):
    return R.rice_parameter(int(np.abs(r).sum()), n - order)


# What EDGE_CASES attains, measured with the restatement, beside what d2d_flac.hip budgets for (has the table).
ATTAINED = dict(
    fixed=FIXED_MAX,                    # max |r| over the five fixed sets: derived, 2^28 - 16                      (budget: |r| < 2^30)
    lpc={4: 21331967, 8: 24173567, 12: 25232895},      # max |r| under each LPC order: 2^24.3 .. 2^24.6             (budget: |r| < 2^30)
    set_sum=1098437820480,              # max sum |r| over one residual set = one partition at partition order 0: 2^40.0 (budget: < 2^48)
    k=28,                               # the largest Rice parameter of any set                                      (cap: 30)
    r0=153910608913727488,              # the largest R(0): 2^57.1                                                   (about 2^58)
    wave=56569089439907968,             # the largest sum of y^2 over one wave's 256 samples: 2^55.65                (budget: < 2^56)
)


SHIFTS = set(range(8, 16))               # the coefficient shifts of its candidates


def c_depth(name):
    return EDGE_CASES[EDGE_IDS.index(name)]["depth"]


@functools.lru_cache(maxsize=None)
def measured():
    """what the corpus attains, and the autocorrelations of its searched signals"""
    fixed, lpc, set_sum, k, r0, wave, r13s = 0, {4: 0, 8: 0, 12: 0}, 0, 0, 0, 0, []
    for i, c in enumerate(EDGE_CASES):
        for info in restated(i)[3]:
            for pl in info["plans"]:
                x, n = pl["x"], len(pl["x"])
                for o, r in enumerate(fixed_sets(x)):
                    fixed = max(fixed, int(np.abs(r).max()))
                    set_sum, k = max(set_sum, int(np.abs(r).sum())), max(k, _k(r, n, o))
                sets, r13 = lpc_sets(x)
                r13s.append(r13)
                for m, r in sets.items():
                    lpc[m] = max(lpc[m], int(np.abs(r).max()))
                    set_sum, k = max(set_sum, int(np.abs(r).sum())), max(k, _k(r, n, m))
                k = max(k, max(pl["ks"]))
                r0 = max(r0, r13[0])
                idx = np.arange(n, dtype=np.int64)
                y = (x * ((idx + 1) * (n - idx))) >> P.window_shift(n)
                wave = max(wave, max(int(np.dot(y[a:a + 256], y[a:a + 256])) for a in range(0, n, 256)))
    return dict(fixed=fixed, lpc=lpc, set_sum=set_sum, k=k, r0=r0, wave=wave), r13s


def test_the_cases_reach_the_kernels_bounds():
    by = {c["name"]: restated(i)[3] for i, c in enumerate(EDGE_CASES)}
    plans = lambda name: [pl for info in by[name] for pl in info["plans"]]
    # the anti-phase side signal and its order-4 difference
    side = by["antiphase"][0]["plans"][3]
    assert side["bits"] == 25 and int(np.abs(side["x"]).min()) == SIDE_MAX and int(np.abs(fixed_sets(side["x"])[4]).max()) == FIXED_MAX
    assert FIXED_MAX == (1 << 28) - 16
    # what the corpus attains: the fixed figure derived, the others as measured
    got = measured()[0]
    assert got == ATTAINED, got
    assert got["fixed"] < 1 << 30 and max(got["lpc"].values()) < 1 << 30 and got["set_sum"] < 1 << 48 and got["k"] <= 30
    assert got["r0"] < 1 << 62 and got["wave"] < 1 << 56
    # how rule 13 ended, per signal
    for name in ("impulse-first", "impulse-middle"):
        assert [(pl["ended"], pl["dropped"], pl["lpc_costs"]) for pl in plans(name)] == [("full", [4, 8, 12], {})] * 2      # cmax == 0
    assert [(pl["ended"], pl["dropped"], sorted(pl["lpc_costs"])) for pl in plans("impulses-5-apart")] == [("full", [4], [8, 12])] * 2
    assert [(pl["ended"], pl["dropped"], sorted(pl["lpc_costs"])) for pl in plans("impulses-11-apart")] == [("full", [4, 8], [12])] * 2
    for name in ("poles+0.9", "poles-0.9"):                          # the drop at sum |q| > 62 * 2^shift: every |a| is below 2^13 here
        (pl,) = plans(name)
        assert (pl["ended"], pl["dropped"], sorted(pl["lpc_costs"])) == ("full", [8, 12], [4]) and pl["lpc"] is not None
    ended = {pl["ended"] for name in by for pl in plans(name)}
    # ("stopped", m) needs |k| >= 1 after rounding.  The window keeps the autocorrelation matrix of any PCM well inside positive
    # definite: neither this corpus nor a seeded search (4000 signals of 64 to 259 samples: poles() with up to twelve reflection
    # coefficients of up to 1 - 2^-20, random rails, squares of periods up to 39, up to four impulses) met it, so no case pins it.
    # VECTORS below runs that branch on the routine itself, on the host and on the device.
    assert ended == {"full"}, ended
    for name in ("poles+0.9", "poles-0.9"):
        assert [m for m, cmax in reached(P.autocorrelation(plans(name)[0]["x"])) if cmax < 8192.0] == [4, 8, 12]
    # the shifts: of the orders rule 16 chose, and of every candidate (the kernel computes them all).  A shift below 7 needs
    # cmax >= 64, and then sum |q| > 62 * 2^shift drops the candidate; 7 needs one coefficient of 32 to 64 beside eleven that add up
    # to less than 30, which neither a signal nor a vector of section 4 gave
    shifts = {pl["sh"] for name in by for pl in plans(name) if pl["lpc_costs"]}
    all_shifts = {sh for r13 in measured()[1] for _, sh in P.coefficients(r13)[0].values()}
    assert shifts == all_shifts == SHIFTS, (shifts, all_shifts)
    assert {pl["sh"] for pl in plans("tiny")} == {15} and {pl["sh"] for pl in plans("poles-0.9-1000")} == {8}
    # every stereo assignment with an LPC subframe, on rail-level input; mid/side with the 25-bit side subframe LPC
    modes = {}
    for name in ("antiphase", "antiphase-64", "near-rails-0", "near-rails-1", "two-squares"):
        info = by[name][0]
        assert any(pl["lpc"] is not None for pl in info["subs"]) and int(np.abs(info["plans"][0]["x"]).min()) >= rails(c_depth(name))[0] - 40
        modes[name] = info["mode"]
    assert modes == {"antiphase": "independent", "antiphase-64": "mid/side", "near-rails-0": "left/side", "near-rails-1": "side/right",
                     "two-squares": "independent"}, modes
    side = by["antiphase-64"][0]["subs"][1]
    assert side["lpc"] is not None and side["bits"] == 25 and int(np.abs(side["x"]).min()) == SIDE_MAX
    # the shapes, the lengths, the periods, the frame numbers
    assert EDGE_GROUPS == sorted(SHAPES)
    for family in ("rails", "squares", "dc"):
        assert sorted((c["samples"].shape[1], c["depth"]) for c in EDGE_CASES if c["name"].startswith(family + "-")) == sorted(SHAPES)
    top = lambda c: rails(c["depth"])
    assert all(set(np.unique(c["samples"])) <= set(top(c)) for c in EDGE_CASES if c["name"].split("-")[0] in ("rails", "squares", "dc", "antiphase"))
    assert {int(v) for c in EDGE_CASES if c["name"].startswith("dc-1ch") for v in np.unique(c["samples"])} == {rails(16)[0], rails(20)[1], rails(24)[0]}
    lengths = {min(B, c["samples"].shape[0] - a) for c in EDGE_CASES for a in range(0, c["samples"].shape[0], B)}
    assert {B, 64, 65, 67, 1000} <= lengths and any(n % 4 for n in lengths)
    assert {len(R.utf8_number(c["first_block"])) for c in EDGE_CASES} >= {1, 2, 3, 4, 5}
    assert sum(len(R.utf8_number(c["first_block"])) < len(R.utf8_number(c["first_block"] + 1)) for c in EDGE_CASES if c["samples"].shape[0] > B) >= 5
    assert any(not c["final"] for c in EDGE_CASES)


def test_the_squares_have_every_period():
    seen = set()
    for c in EDGE_CASES:
        if c["name"].startswith("squares-"):
            for ch in range(c["samples"].shape[1]):
                x = c["samples"][:B, ch]
                seen.add(next(p for p in range(2, 27) if np.array_equal(x[p:], x[:-p])))
    assert seen == set(PERIODS), seen


@pytest.mark.parametrize("i", range(len(EDGE_CASES)), ids=EDGE_IDS)
def test_host_equals_the_restatements_on_the_edge_cases(engine_lib, i):
    c = EDGE_CASES[i]
    s, depth = c["samples"], c["depth"]
    want, sizes, used, _ = restated(i)
    got, res, consumed = engine_lib.flac_encode_host(s.shape[1], depth, R.pack_pcm(s, depth), first_block=c["first_block"], final=c["final"], effort=12)
    assert got == want
    assert (res.bytes_out, res.min_frame_bytes, res.max_frame_bytes, consumed) == (sum(sizes), min(sizes), max(sizes), used)
    for b, fs in enumerate(sizes):                                   # every frame stays within the bound
        assert fs <= R.frame_bound(s.shape[1], depth, min(B, s.shape[0] - B * b)), b
    for effort in EFFORTS:                                           # effort 1 against its restatement; both through the decoder
        check_host(engine_lib, s, depth, effort, first_block=c["first_block"], final=c["final"], restated=effort == 1)


# ---- 3. the host verifier on what the host encoder made of EDGE_CASES ----------------------------------------------------------------
SERIAL, COOP = 1, 2


@pytest.mark.parametrize("effort", EFFORTS)
def test_the_verifier_accepts_the_edge_cases(engine_lib, effort):
    d = engine_lib
    for c in EDGE_CASES:
        s, depth, ch = c["samples"], c["depth"], c["samples"].shape[1]
        pcm = R.pack_pcm(s, depth)
        frames, _, used = d.flac_encode_host(ch, depth, pcm, first_block=c["first_block"], final=c["final"], effort=effort)
        sizes = frame_sizes(d, ch, depth, pcm[:used * (pcm.size // s.shape[0])], effort, c["first_block"])
        assert sum(sizes) == len(frames)
        for method in (SERIAL, COOP):
            st = d.FlacVerifyStats()
            v = d.flac_verify_host(ch, depth, pcm, frames, first_block=c["first_block"], final=c["final"], sizes=sizes, method=method, stats=st)
            assert v.as_tuple() == clean(used, nblocks(used)), (c["name"], method, v.as_tuple())
            assert st.as_tuple() == ((0, nblocks(used)) if method == SERIAL else (nblocks(used), 0)), (c["name"], method, st.as_tuple())


@pytest.mark.parametrize("effort", EFFORTS)
def test_the_verifier_sees_one_flipped_bit_in_a_rail_level_block(engine_lib, effort):
    d = engine_lib
    c = EDGE_CASES[EDGE_IDS.index("antiphase")]
    s = c["samples"]
    frames = d.flac_encode_host(2, 24, R.pack_pcm(s, 24), first_block=c["first_block"], effort=effort)[0]
    sizes = frame_sizes(d, 2, 24, R.pack_pcm(s, 24), effort, c["first_block"])
    for index, channel in ((17, 1), (B + 999, 0)):
        x = s.copy()
        x[index, channel] ^= 1
        for method in (SERIAL, COOP):
            st = d.FlacVerifyStats()
            v = d.flac_verify_host(2, 24, R.pack_pcm(x, 24), frames, first_block=c["first_block"], sizes=sizes, method=method, stats=st)
            assert st.as_tuple() == ((0, 2) if method == SERIAL else (1, 1))      # the cooperative rule accepts the other block only
            assert v.as_tuple() == (s.shape[0] - (B if index < B else 1000), 2, 1, index // B, BAD_SAMPLES), (index, method, v.as_tuple())


# ---- 4. rule 13 itself: VECTORS ---------------------------------------------------------------------------------------------------------
# Thirteen integers each.  lpc_coefficients is total for any R(0) > 0 (and answers "no candidates" for R(0) == 0), so nothing is left out.

def _seeded_vectors():
    g = np.random.default_rng(2026)
    out = []
    # the stop branch on both sides of its rounding edge: a reflection coefficient of +/- (1 - 2^-j) at order m, small ones in front.
    # 1 - k^2 rounds to something positive as long as k is not +/- 1 as a double; the division that makes k rounds, so which side a
    # vector falls on is the restatement's to say
    for j in range(1, 53):
        for m in (1, 4, 5, 9, 12):
            for sign in (1, -1):
                ks = [Fraction(int(g.integers(-3, 4)), 10) for _ in range(m - 1)] + [sign * (1 - Fraction(1, 1 << j))]
                ks += [Fraction(int(g.integers(-5, 6)), 10) for _ in range(12 - m)]
                out.append(from_reflection(ks, scale=1 << int(g.integers(20, 62))))
    # coefficient magnitudes on both sides of 2^13 and sums on both sides of 62 * 2^shift: all reflection coefficients +/- the same
    # value near one give coefficients like binomials, whose size the value tunes
    for t in range(600):
        v = Fraction(int(g.integers(500, 1000)), 1000) * (-1 if t % 2 else 1)
        ks = [v if (t // 2) % 3 != 2 or m % 2 else -v for m in range(12)]
        if t % 5 == 0:
            ks = [Fraction(int(g.integers(-2, 3)), 10)] * int(g.integers(1, 8)) + ks
        out.append(from_reflection(ks[:12], scale=1 << int(g.integers(30, 62))))
    # any reflection coefficients; R(0) from 1 to 2^62
    for t in range(800):
        ks = [Fraction(int(g.integers(-999, 1000)), 1000) for _ in range(12)]
        out.append(from_reflection(ks, scale=1 << int(g.integers(0, 63))))
    # integers that are nobody's autocorrelation: the recursion stops, or goes on with coefficients of any size
    for t in range(800):
        top = 1 << int(g.integers(1, 63))
        r0 = int(g.integers(1, top, endpoint=True))
        spread = (1.0, 0.5, 0.1, 1.5)[t % 4]
        out.append([r0] + [int(v) for v in np.clip(np.rint(g.uniform(-spread, spread, 12) * r0), -(1 << 62), 1 << 62)])
    # all twelve reflection coefficients at +/- (1 - 2^-j): coefficients towards the binomial coefficients, the largest there are
    out += [from_reflection([sign * (1 - Fraction(1, 1 << j))] * 12, scale=1 << 60) for j in (3, 4, 5) for sign in (1, -1)]
    out.append([1 << 62] + [0] * 12)
    out.append([1 << 62] + [(1 << 62) - l * l for l in range(1, 13)])
    out.append([1] + [0] * 12)
    return out


@functools.lru_cache(maxsize=None)
def vectors():
    """[(name, thirteen Python ints)]: HAND, the autocorrelations of EDGE_CASES's signals (each once), the seeded set"""
    corpus = sorted({tuple(r13) for r13 in measured()[1]})
    return ([("hand-" + k, list(HAND[k][0])) for k in sorted(HAND)] + [("corpus-%d" % i, list(v)) for i, v in enumerate(corpus)] +
            [("seeded-%d" % i, v) for i, v in enumerate(_seeded_vectors())])


@functools.lru_cache(maxsize=None)
def vectors_restated():
    """[({P: (q, shift)}, ended, dropped)] of vectors() by flac_lpc_ref.coefficients"""
    return [P.coefficients(v) for _, v in vectors()]


def run_probe(exe, vecs, tmp_path, timeout=120):
    """the probe's answer to [(name, vector)]: [{P: (q, shift)}], one per vector"""
    path = os.path.join(str(tmp_path), "vectors.txt")
    with open(path, "w") as f:
        f.write("\n".join(" ".join(str(x) for x in v) for _, v in vecs) + "\n")
    p = subprocess.run([exe, path], capture_output=True, text=True, timeout=timeout)
    assert p.returncode == 0, p.stderr
    lines = p.stdout.splitlines()
    assert len(lines) == 3 * len(vecs)
    out = []
    for at in range(0, len(lines), 3):
        one = {}
        for line, order in zip(lines[at:at + 3], P.ORDERS):
            f = line.split()
            assert int(f[0]) == order
            if f[1] != "none":
                one[order] = ([int(v) for v in f[2:]], int(f[1]))
        out.append(one)
    return out


def assert_probe_equals_the_restatement(got):
    want = [c for c, _, _ in vectors_restated()]
    wrong = [i for i, (g, w) in enumerate(zip(got, want)) if g != {m: (list(q), sh) for m, (q, sh) in w.items()}]
    assert not wrong, (len(wrong), [(vectors()[i], got[i], want[i]) for i in wrong[:3]])
    assert len(got) == len(want)


def test_the_vectors_fire_every_branch():
    ended = [e if isinstance(e, str) else e[0] for _, e, _ in vectors_restated()]
    counts = {k: ended.count(k) for k in set(ended)}
    dropped = sum(1 for _, e, gone in vectors_restated() if gone)
    full = sum(1 for c, e, gone in vectors_restated() if e == "full" and not gone and len(c) == 3)
    assert (len(vectors()), counts, dropped, full) == VECTOR_COUNTS, (len(vectors()), counts, dropped, full)
    assert counts["stopped"] and dropped and full
    stops = {e[1] for _, e, _ in vectors_restated() if isinstance(e, tuple)}
    assert stops == set(range(1, 13)), stops
    # both sides of 2^13, of 62 * 2^shift and of the stop's rounding edge; R(0) at 2^62
    cmax = [(c.get(m), top) for (_, v), (c, _, _) in zip(vectors(), vectors_restated()) for m, top in reached(v)]
    # No vector can put a coefficient at 2^13: err > 0 at every step means |k| < 1 at every step, and then |a[j]| of order m is below
    # the binomial coefficient (m over j), 924 at most.  The routine's test of |a| < 2^13 never fails behind its test of err; 612 is
    # the largest magnitude here (closer to one than 1 - 2^-5 twelve times over, the recursion in doubles stops).  The drop at
    # sum |q| > 62 * 2^shift does fire: among the candidates with cmax from 8 to 32 some are dropped and some are kept, below 8 most
    # are kept, from 64 on every one is dropped (q alone is then beyond 62 * 2^shift)
    assert 600.0 < max(top for _, top in cmax) < 924.0
    assert sum(1 for c, top in cmax if c is None and 8.0 <= top < 32.0) > 20 and sum(1 for c, top in cmax if c is not None and 8.0 <= top < 32.0) > 20
    assert sum(1 for c, top in cmax if c is None and top >= 64.0) > 20 and not any(c is not None and top >= 64.0 for c, top in cmax)
    assert sum(1 for c, top in cmax if c is not None and top < 8.0) > 20 and sum(1 for c, top in cmax if c is None and top < 8.0) > 20
    assert max(abs(v) for c, _, _ in vectors_restated() for q, _ in c.values() for v in q) == 8192      # the clamp at -2^13
    near_one = [(n, e) for (n, v), (_, e, _) in zip(vectors(), vectors_restated()) if n.startswith("seeded-") and int(n[7:]) < 52 * 10]
    assert {isinstance(e, tuple) for _, e in near_one} == {True, False}
    assert max(v[0] for _, v in vectors()) == 1 << 62 and {sh for c, _, _ in vectors_restated() for _, sh in c.values()} == SHIFTS


# (vectors, how they ended, those with a dropped candidate, those with all three candidates)
VECTOR_COUNTS = (3007, {"full": 2034, "stopped": 972, "silence": 1}, 500, 1572)


@pytest.fixture(scope="module")
def host_probe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("flac_lpc_probe") / "flac_lpc_probe")
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-o", exe, "flac_lpc_probe.cpp"], cwd=os.path.join(ROOT, "tools"),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return exe


def test_the_host_routine_equals_the_restatement_on_the_vectors(host_probe, tmp_path):
    assert_probe_equals_the_restatement(run_probe(host_probe, vectors(), tmp_path))
