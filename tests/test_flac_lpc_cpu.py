"""FLAC effort 12 without a GPU (include/dsd2dxd_amd.h, "EFFORTS"): d2d_flac_encode_host_effort at D2D_FLAC_EFFORT_LPC -- the sink's
frame encoder behind the C ABI and the reference of tests/test_gpu_flac_lpc.py -- against the plain-Python restatement of
flac_lpc_ref.py, byte for byte; the round trip through that file's own decoder; frame for frame effort 12 <= effort 1 <= effort 0;
efforts 0 and 1 unchanged; effort 12 accepted by all three entry points; efforts 3 and 13 refused.

CASES is the input set of both files.  test_the_cases_force_every_decision counts what the restatement chose over the set and fails
if a kind is missing.  The two branches of rule 13 that windowed audio does not reach -- a candidate dropped at
sum |q| > 62 * 2^shift, the recursion stopped at !(err > 0) -- are tested on the routine itself: tools/flac_lpc_probe.cpp, built
here with g++, against the restatement on hand-made autocorrelations."""
import ctypes as C
import functools
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import flac_lpc_ref as P
import flac_ref as R
import flac_search_ref as S
from test_flac_search_cpu import walk, white

BLOCK = R.BLOCK
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LPC = 12


def ar(n, ch, depth, pairs, seed, amp=200.0, rad=0.97, tilt=0.3):
    """white noise through `pairs` resonant pole pairs of radius `rad`, spread over the band (each channel's a little elsewhere): an
    order-2*pairs process, so that 2, 4 and 6 pairs make LPC orders 4, 8 and 12 the cheapest"""
    g = np.random.default_rng(seed)
    out = np.zeros((n, ch), dtype=np.int64)
    for c in range(ch):
        poly = np.array([1.0])
        for k in range(pairs):
            w = np.pi * (k + 1 + tilt * c) / (pairs + 1.5)
            poly = np.convolve(poly, [1.0, -2 * rad * np.cos(w), rad * rad])
        e = g.normal(0, amp, n + 200)
        y = np.zeros(n + 200)
        for i in range(n + 200):
            m = min(i, len(poly) - 1)
            y[i] = e[i] - np.dot(poly[1:m + 1], y[i - m:i][::-1])
        out[:, c] = np.rint(y[200:])
    return R._clip(out, depth)


def lpc_stereo(n, depth, kind, seed):
    """an order-12 process in both channels: left/side and side/right with a small white difference (the side subframe is fixed,
    the other one LPC), mid/side with a coloured difference (an LPC side subframe, one bit wider), independent with unrelated ones"""
    common = ar(n, 1, depth, 6, seed, amp=300.0)[:, 0]
    small = np.random.default_rng(seed + 1).integers(-60, 61, size=n).astype(np.int64)
    if kind == "left/side":
        l, r = common, common + small
    elif kind == "side/right":
        l, r = common + small, common
    elif kind == "mid/side":
        d = ar(n, 1, depth, 4, seed + 2, amp=30.0)[:, 0]
        l, r = common + d, common - d
    else:
        l, r = common, ar(n, 1, depth, 4, seed + 3, amp=20.0)[:, 0]
    return R._clip(np.stack([l, r], axis=1), depth)


def _case(name, samples, depth, first_block=0, final=True):
    return dict(name=name, samples=np.asarray(samples, dtype=np.int64), depth=depth, first_block=first_block, final=final)


def _build_cases():
    cases = []
    # each LPC order, across the depths
    cases += [_case("ar%d" % (2 * p), ar(BLOCK, 1, d, p, p), d) for p, d in ((2, 24), (4, 16), (6, 20))]
    # a fixed plan with LPC candidates present; silence (R(0) == 0); tiny white noise (the shift clamped at 15)
    cases += [_case("white", white(BLOCK, 1, 16, 1), 16), _case("walk2", walk(BLOCK, 1, 24, 3, order=2), 24)]
    cases += [_case("silence", np.zeros((BLOCK, 2)), 24), _case("tiny", np.random.default_rng(4).integers(-4, 5, size=(BLOCK, 1)), 16)]
    # the lengths: 63 is the effort-1 frame, 64 the first with LPC; a short block with pmax 3; a last block of 4095; three blocks
    # (so short a frame pays for four coefficients only where the poles are strong)
    cases += [_case("ar4-%d" % n, ar(n, 1, 24, 2, n, amp=2000.0, rad=0.99), 24) for n in (63, 64, 65)]
    cases += [_case("ar12-%d" % n, ar(n, 1, 24, 6, n), 24) for n in (1000, 4095)]
    cases.append(_case("ar8-3blocks", ar(2 * BLOCK + 1000, 2, 16, 4, 9), 16, 0x7F))
    cases.append(_case("ar12-not-final", ar(BLOCK + 500, 1, 20, 6, 10), 20, 0x7FF, False))
    # every stereo assignment with an LPC subframe in it; mid/side at depth 24 has the 25-bit LPC side subframe
    cases += [_case("stereo-" + k, lpc_stereo(BLOCK, d, k, 20 + i), d) for i, (k, d) in enumerate(zip(S.MODES, (16, 20, 24, 24)))]
    # the channel counts
    cases += [_case("ar12-3ch", ar(1000, 3, 24, 6, 30), 24), _case("ar8-8ch", ar(BLOCK + 64, 8, 24, 4, 31, tilt=0.05), 24, 0xFFFF)]
    # exact ties, where a search of seeds with the restatement finds one (TIES)
    cases += [_case("tie-%s-%d" % (kind, seed), tie_signal(seed), 16) for kind, seed in TIES]
    return cases


def tie_signal(seed):
    """the short coloured noises a seeded search was run over"""
    g = np.random.default_rng(seed)
    n = int(g.choice([64, 65, 80, 96, 128]))
    amp = int(g.choice([3, 6, 12, 30, 100]))
    w = g.integers(-amp, amp + 1, size=n + 4).astype(np.int64)
    kind = seed % 3
    if kind == 0:
        x = w[4:] + w[3:-1] - w[1:-3]
    elif kind == 1:
        x = np.cumsum(w)[4:] - np.cumsum(w)[:-4]
    else:
        x = w[4:] * 2 - w[2:-2] + w[:-4]
    return x.reshape(-1, 1)


TIES = ()            # (("order" | "cost", seed), ...) of tie_signal: none was found, see test_the_cases_force_every_decision
CASES = _build_cases()
IDS = [c["name"] for c in CASES]


@functools.lru_cache(maxsize=None)
def restated(i):
    """(bytes, sizes, consumed, infos) of case i by the restatement: computed once, shared by the tests of both files"""
    c = CASES[i]
    return P.encode(c["samples"], c["depth"], first_block=c["first_block"], final=c["final"])


def host(engine_lib, c, effort):
    s = c["samples"]
    return engine_lib.flac_encode_host(s.shape[1], c["depth"], R.pack_pcm(s, c["depth"]), first_block=c["first_block"], final=c["final"], effort=effort)


def test_the_cases_force_every_decision():
    chosen, fixed_with_candidates, silence, shifts, modes_with_lpc, depths, channels = set(), 0, 0, set(), set(), set(), set()
    lpc_side_25 = tie_order = tie_cost = False
    for i, c in enumerate(CASES):
        for info in restated(i)[3]:
            if info["mode"] is None:
                continue
            for pl in info["plans"]:                                # every candidate signal's search
                if pl["ended"] == "silence":
                    silence += 1
                if pl["lpc_costs"]:
                    shifts.add(pl["sh"])
                    lc = pl["lpc_costs"]
                    if list(lc.values()).count(min(lc.values())) > 1:
                        tie_order = True
                        assert pl["lpc_order"] == min(o for o in lc if lc[o] == min(lc.values()))      # the smaller order
                    if pl["cost2"] == pl["cost1"]:
                        tie_cost = True
                        assert pl["lpc"] is None                    # the effort-1 plan stays
                    assert (pl["lpc"] is not None) == (pl["cost2"] < pl["cost1"])
                    if pl["lpc"] is None:
                        fixed_with_candidates += 1
            subs = info["subs"]                                     # what was written
            for pl in subs:
                if pl["lpc"] is not None:
                    chosen.add(pl["order"])
                    depths.add(c["depth"])
                    channels.add(c["samples"].shape[1])
            if any(pl["lpc"] is not None for pl in subs):
                modes_with_lpc.add(info["mode"])
            if info["mode"] in ("left/side", "mid/side") and subs[1]["lpc"] is not None and subs[1]["bits"] == 25:
                lpc_side_25 = True
    assert chosen == {4, 8, 12}
    assert fixed_with_candidates and silence
    assert 15 in shifts and len(shifts) > 1
    assert modes_with_lpc == set(S.MODES) and lpc_side_25
    assert depths == {16, 20, 24} and channels == {1, 2, 3, 8}
    # ties: a seeded search with the restatement (tie_signal over seeds 0 .. 199999) met neither two LPC orders of equal cost nor
    # cost2 == cost1, so no case pins one; both rules are asserted above wherever the set meets them, and a tie that TIES names is met
    assert all({"order": tie_order, "cost": tie_cost}[k] for k, _ in TIES)
    # what the named cases are there for
    by = {c["name"]: restated(i)[3] for i, c in enumerate(CASES)}
    assert [by["ar%d" % o][0]["subs"][0]["order"] for o in (4, 8, 12)] == [4, 8, 12]
    assert all(by[k][0]["subs"][0]["lpc"] is None and by[k][0]["plans"][0]["lpc_costs"] for k in ("white", "walk2"))
    assert by["tiny"][0]["plans"][0]["sh"] == 15
    assert by["ar4-63"][0]["mode"] is None and restated(IDS.index("ar4-63"))[0] == S.encode(CASES[IDS.index("ar4-63")]["samples"], 24)[0]
    assert all(by[k][0]["subs"][0]["lpc"] is not None for k in ("ar4-64", "ar4-65", "ar12-1000", "ar12-4095"))
    assert [by["stereo-" + k][0]["mode"] for k in S.MODES] == list(S.MODES)
    assert len(by["ar8-3blocks"]) == 3 and len(by["ar12-not-final"]) == 1
    assert {c["samples"].shape[0] for c in CASES} >= {63, 64, 65, 1000, 4095}


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_host_effort_12_equals_the_restatement(engine_lib, i):
    c = CASES[i]
    want, sizes, used, _ = restated(i)
    got, res, consumed = host(engine_lib, c, LPC)
    assert got == want
    assert (res.bytes_out, res.min_frame_bytes, res.max_frame_bytes) == (sum(sizes), min(sizes, default=0), max(sizes, default=0))
    assert consumed == used


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_effort_12_decodes_to_the_input_and_is_never_longer(engine_lib, i):
    c = CASES[i]
    s = c["samples"]
    got, _, consumed = host(engine_lib, c, LPC)
    back, sizes, infos = P.decode(got, s.shape[1], c["depth"], first_block=c["first_block"])      # (asserts every CRC-8 and CRC-16)
    assert np.array_equal(back, s[:consumed])
    # the decoder read the choices the restatement made
    for seen, f in zip(infos, restated(i)[3]):
        if f["mode"]:
            want = [("lpc" if pl["lpc"] is not None else "fixed", pl["order"], pl["porder"]) for pl in f["subs"]]
            assert seen == (S.MODE_NIBBLE.get(f["mode"], s.shape[1] - 1), want)
    # frame for frame: effort 12 <= effort 1 <= effort 0
    one = P.decode(host(engine_lib, c, 1)[0], s.shape[1], c["depth"], first_block=c["first_block"])[1]
    plain = R.encode(s, c["depth"], first_block=c["first_block"], final=c["final"])[1]
    assert len(sizes) == len(one) == len(plain)
    assert all(a <= b <= z for a, b, z in zip(sizes, one, plain))


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_efforts_0_and_1_through_the_same_entry_are_unchanged(engine_lib, i):
    c = CASES[i]
    s = c["samples"]
    assert host(engine_lib, c, 0)[0] == R.encode(s, c["depth"], first_block=c["first_block"], final=c["final"])[0]
    assert host(engine_lib, c, 1)[0] == S.encode(s, c["depth"], first_block=c["first_block"], final=c["final"])[0]


def test_effort_12_is_accepted_by_all_three_entry_points(engine_lib):
    """the device entry and the stream driver check the effort first and answer on the host, before any device call: with effort 12
    they go on to refuse what is wrong with the rest of these calls -- no files, no engine -- and not the effort"""
    L = engine_lib.lib()
    assert engine_lib.FLAC_EFFORT_LPC == LPC
    s = ar(BLOCK + 10, 2, 24, 6, 1)
    got, res, used = engine_lib.flac_encode_host(2, 24, R.pack_pcm(s, 24), effort=LPC)
    assert res.bytes_out == len(got) > 0 and used == BLOCK + 10
    assert L.d2d_flac_encode_device_effort(2, 24, LPC, None, 0, None, 0, None) == -1
    assert b"effort" not in L.d2d_flac_error() and b"no files" in L.d2d_flac_error()
    stats = engine_lib.FlacStreamStats(1, 2, 3, 4)
    assert L.d2d_convert_stream_flac_effort(None, 24, LPC, engine_lib._capi.READ_FN(), None, engine_lib._capi.WRITE_FN(), None, None,
                                            engine_lib._capi.PROGRESS_FN(), None, 0, 0, C.byref(stats)) == -1
    assert b"effort" not in L.d2d_flac_error() and b"null engine" in L.d2d_flac_error()


def test_efforts_3_and_13_are_refused_with_nothing_written(engine_lib):
    L = engine_lib.lib()
    s = R.signal("sine", BLOCK + 10, 2, 24)
    pcm = R.pack_pcm(s, 24)
    cap = engine_lib.flac_bound_bytes(2, 24, BLOCK + 10, 1)
    for effort in (3, 11, 13):
        out = np.full(cap, 0xA5, dtype=np.uint8)
        res, used = engine_lib.FlacResult(111, 222, 333), C.c_size_t(444)
        rc = L.d2d_flac_encode_host_effort(2, 24, effort, pcm.ctypes.data, BLOCK + 10, 0, 1, out.ctypes.data, cap, C.byref(res), C.byref(used))
        assert rc == -1 and b"effort" in L.d2d_flac_error()
        assert (out == 0xA5).all() and (res.bytes_out, res.min_frame_bytes, res.max_frame_bytes, used.value) == (111, 222, 333, 444)
        x = engine_lib.FlacIO()
        x.pcm, x.frames, x.final, x.out, x.out_capacity_bytes, x.result, x.blocks, x.frames_consumed = 0x10000, BLOCK + 10, 1, 0x20000, cap, 0x30000, 777, 888
        ios = (engine_lib.FlacIO * 1)(x)
        ws = engine_lib.flac_workspace_bytes(2, 24, BLOCK + 10, 1)
        assert L.d2d_flac_encode_device_effort(2, 24, effort, ios, 1, C.c_void_p(0x40000), ws, None) == -1 and b"effort" in L.d2d_flac_error()
        assert (ios[0].blocks, ios[0].frames_consumed) == (777, 888)
        stats = engine_lib.FlacStreamStats(1, 2, 3, 4)
        assert L.d2d_convert_stream_flac_effort(None, 24, effort, engine_lib._capi.READ_FN(), None, engine_lib._capi.WRITE_FN(), None, None,
                                                engine_lib._capi.PROGRESS_FN(), None, 0, 0, C.byref(stats)) == -1
        assert b"effort" in L.d2d_flac_error() and (stats.samples_per_channel, stats.blocks) == (1, 2)


# ---- rule 13 on hand-made autocorrelations ---------------------------------------------------------------------------------------------

def from_reflection(ks, scale=1 << 56):
    """the autocorrelation whose recursion meets the reflection coefficients ks: exact rationals, scaled and rounded"""
    r, a, err = [Fraction(1)], [Fraction(0)] * 13, Fraction(1)
    for m, k in enumerate(ks, 1):
        r.append(k * err + sum(a[j] * r[m - j] for j in range(1, m)))
        new = list(a)
        for j in range(1, m):
            new[j] = a[j] - k * a[m - j]
        new[m] = k
        a, err = new, err * (1 - k * k)
    return [int(round(v * scale)) for v in r]


def _noise_r():
    y = [int(v) for v in np.random.default_rng(1).integers(-1000, 1001, size=512)]
    return [sum(y[i] * y[i - l] for i in range(l, len(y))) for l in range(13)]


NINE_TENTHS = Fraction(9, 10)
HAND = {
    # reflection coefficients near one make coefficients like binomials: sum |q| > 62 * 2^shift from order 8 on, or at order 12 alone
    "drop-8-12": (from_reflection([-NINE_TENTHS] * 12), "full", [8, 12]),
    "drop-12": (from_reflection([NINE_TENTHS] * 12), "full", [12]),
    "drop-late": (from_reflection([Fraction(1, 10)] * 4 + [-NINE_TENTHS] * 8), "full", [12]),
    # k == 1 at once: err == 0; k > 1: err < 0; the same after orders 4 and 8 were reached
    "stop-1-zero": ([1 << 40] * 13, ("stopped", 1), []),
    "stop-1-negative": ([4, 5] + [0] * 11, ("stopped", 1), []),
    "stop-5": (_noise_r()[:5] + [2 * _noise_r()[0]] + _noise_r()[6:], ("stopped", 5), []),
    "stop-9": (_noise_r()[:9] + [-3 * _noise_r()[0]] + _noise_r()[10:], ("stopped", 9), []),
    "noise": (_noise_r(), "full", []),
    "silence": ([0] * 13, "silence", []),
    "largest": ([1 << 60] + [(1 << 60) - 3 * l * l for l in range(1, 13)], None, None),
}


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("flac_lpc_probe") / "flac_lpc_probe")
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-o", exe, "flac_lpc_probe.cpp"], cwd=os.path.join(ROOT, "tools"),
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

    def run(R13):
        p = subprocess.run([exe] + [str(v) for v in R13], capture_output=True, text=True, timeout=60)
        assert p.returncode == 0, p.stderr
        out = {}
        for line in p.stdout.splitlines():
            f = line.split()
            if f[1] != "none":
                out[int(f[0])] = ([int(v) for v in f[2:]], int(f[1]))
        return out
    return run


@pytest.mark.parametrize("name", sorted(HAND))
def test_the_routine_equals_the_restatement_on_hand_made_autocorrelations(probe, name):
    R13, ended, dropped = HAND[name]
    want, how, gone = P.coefficients(R13)
    if ended is not None:
        assert (how, gone) == (ended, dropped)                      # the branch this vector is there to fire
        stopped_at = how[1] if isinstance(how, tuple) else 13
        assert sorted(want) == [m for m in P.ORDERS if m < stopped_at and m not in gone] if how != "silence" else want == {}
    got = probe(R13)
    assert got == {m: (list(q), sh) for m, (q, sh) in want.items()}
    for q, sh in got.values():
        assert sum(abs(v) for v in q) <= 62 << sh and all(-8192 <= v <= 8191 for v in q) and 0 <= sh <= 15
