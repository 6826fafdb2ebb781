"""FLAC effort 1 without a GPU (include/dsd2dxd_amd.h, "EFFORTS"): d2d_flac_encode_host_effort -- the sink's frame encoder behind
the C ABI and the reference of tests/test_gpu_flac_search.py -- against the plain-Python restatement of flac_search_ref.py, byte for
byte; the round trip through that file's decoder; effort 1 never longer than effort 0; effort 0 unchanged; an unknown effort refused.

CASES is the input set of both files.  test_the_cases_force_every_decision asserts that, over the set, the restatement chooses every
predictor order, every partition order and every channel assignment, and meets an exact tie of each kind."""
import ctypes as C
import functools

import numpy as np
import pytest

import flac_ref as R
import flac_search_ref as S

BLOCK = R.BLOCK


def _rng(seed):
    return np.random.default_rng(seed)


def white(n, ch, depth, seed):
    """order 0 wins: uniform noise, no correlation between samples"""
    return R.noise(n, ch, depth, depth - 3, seed)


def walk(n, ch, depth, seed, order=1):
    """order 1 (2) wins: noise integrated once (twice); the steps are small enough for the depth"""
    a = 40 if order == 1 else 20
    s = _rng(seed).integers(-a, a + 1, size=(n, ch)).astype(np.int64)
    for _ in range(order):
        s = np.cumsum(s, axis=0)
    return R._clip(s, depth)


def slow_sine(n, ch, depth, period):
    """orders 3 and 4 win: a full-scale sine so slow that differencing keeps paying until the rounding noise takes over"""
    i = np.arange(n, dtype=np.float64)[:, None]
    c = np.arange(ch, dtype=np.float64)[None, :]
    return np.rint(((1 << (depth - 1)) - 1) * np.sin(2 * np.pi * i / period + 0.9 * c)).astype(np.int64)


def step(n, ch, depth, p, seed):
    """partition order p wins: quiet noise, loud in the second partition of order p alone.  p = 0: one magnitude with random signs,
    so that every partition of every order has the same mean and the same k, and splitting only adds parameters"""
    s = _rng(seed).integers(-3, 4, size=(n, ch)).astype(np.int64)
    loud = _rng(seed + 1).integers(-(1 << (depth - 3)), 1 << (depth - 3), size=(n, ch)).astype(np.int64)
    if p == 0:
        return 1000 * (2 * _rng(seed).integers(0, 2, size=(n, ch)).astype(np.int64) - 1)
    psz = n >> p
    s[psz:2 * psz] = loud[psz:2 * psz]
    return s


def stereo(n, depth, kind, seed):
    """left/side: R = L + small noise; side/right: L = R + small noise; mid/side: common plus small independent parts; independent:
    a loud and a quiet channel with nothing in common.  The common part is a walk and the small parts are white, so the channel that
    carries the small part on top of the walk is the dearer one of the two, and the side channel is cheaper than either."""
    rng = _rng(seed)
    common = np.cumsum(rng.integers(-200, 201, size=n)).astype(np.int64)
    small = lambda a: rng.integers(-a, a + 1, size=n).astype(np.int64)
    if kind == "left/side":
        l = common
        r = l + small(60)
    elif kind == "side/right":
        r = common
        l = r + small(60)
    elif kind == "mid/side":
        l, r = common + small(40), common + small(40)
    else:
        l, r = small(1 << (depth - 3)), small(3)
    return R._clip(np.stack([l, r], axis=1), depth)


def tiny(n, ch, seed, amp=2):
    return _rng(seed).integers(-amp, amp + 1, size=(n, ch)).astype(np.int64)


def two_level(half, a1, a2, seed):
    g = _rng(seed)
    return np.concatenate([g.integers(-a1, a1 + 1, size=(half, 1)), g.integers(-a2, a2 + 1, size=(half, 1))]).astype(np.int64)


def _case(name, samples, depth, first_block=0, final=True):
    return dict(name=name, samples=np.asarray(samples, dtype=np.int64), depth=depth, first_block=first_block, final=final)


def _build_cases():
    cases = []
    # every predictor order
    cases += [_case("white", white(BLOCK, 1, 16, 1), 16), _case("walk", walk(BLOCK, 1, 20, 2), 20), _case("walk2", walk(BLOCK, 1, 24, 3, order=2), 24)]
    cases += [_case("sine%d" % p, slow_sine(BLOCK, 1, 24, p), 24) for p in ORDER_SINES]
    # every partition order
    cases += [_case("step%d" % p, step(BLOCK, 1, 16, p, 10 + p), 16) for p in range(7)]
    # every channel assignment, across the depths
    cases += [_case("stereo-" + k, stereo(BLOCK, d, k, 20 + i), d) for i, (k, d) in
              enumerate(zip(S.MODES, (24, 16, 20, 24)))]
    # exact ties: found by searching seeds with the restatement, pinned by test_the_cases_force_every_decision
    cases.append(_case("tie-order", tiny(16, 1, TIE_ORDER_SEED), 16))
    cases.append(_case("tie-partition", two_level(16, 1, 5, TIE_PART_SEED), 16))
    equal = walk(1024, 1, 24, 5)
    cases.append(_case("tie-assignment", np.concatenate([equal, equal], axis=1), 24))          # L == R: M == L, S == 0
    cases.append(_case("silence-order-0", np.zeros((64, 1)), 16))
    # the signals of the effort-0 tests over the lengths, channel counts and depths; frame numbers across UTF-8 length boundaries
    grid = [("silence", 15, 1, 16, 0, True), ("random", 15, 2, 24, 3, True), ("random", 16, 2, 16, 0, True), ("sine", 16, 3, 24, 0, True),
            ("spike", 17, 2, 20, 0, True), ("random", 17, 8, 24, 0, True), ("alternate", 32, 2, 24, 0, True), ("sine", 32, 1, 16, 0, True),
            ("sine", 1024, 2, 24, 0, True), ("spike", 1024, 3, 16, 0, True), ("alternate", BLOCK, 8, 24, 0, True), ("silence", BLOCK, 2, 20, 0, True),
            ("sine", BLOCK + 1000, 2, 16, 0x7F, True), ("random", BLOCK + 1000, 3, 20, 0x7FF, True), ("spike", BLOCK + 1000, 1, 24, 0, True),
            ("sine", 4095, 2, 24, 0, False), ("sine", 2 * BLOCK + 1000, 8, 24, 0xFFFF, True), ("sine", 2 * BLOCK + 1000, 2, 20, 0x7F - 1, True),
            ("sine", BLOCK + 8, 2, 24, 0, True), ("random", BLOCK + 2, 2, 16, 0, True)]
    cases += [_case(f"{sig}-{n}-{ch}ch", R.signal(sig, n, ch, d, seed=n + ch), d, fb, fin) for sig, n, ch, d, fb, fin in grid]
    return cases


ORDER_SINES = (4000, 700)            # periods, in samples, of the full-scale sines that orders 3 and 4 win
TIE_ORDER_SEED, TIE_PART_SEED = 0, 28
CASES = _build_cases()
IDS = [c["name"] for c in CASES]


@functools.lru_cache(maxsize=None)
def restated(i):
    """(bytes, sizes, consumed, infos) of case i by the restatement: computed once, shared by the tests of both files"""
    c = CASES[i]
    return S.encode(c["samples"], c["depth"], first_block=c["first_block"], final=c["final"])


def host(engine_lib, c, effort):
    s = c["samples"]
    return engine_lib.flac_encode_host(s.shape[1], c["depth"], R.pack_pcm(s, c["depth"]), first_block=c["first_block"], final=c["final"], effort=effort)


def test_the_cases_force_every_decision():
    orders, porders, modes = set(), set(), set()
    tie_order = tie_part = tie_mode = False
    for i in range(len(CASES)):
        for info in restated(i)[3]:
            if info["mode"] is None:
                continue
            orders.update(info["orders"])
            porders.update(info["porders"])
            modes.add(info["mode"])
            for o, p, oc, pc in zip(info["orders"], info["porders"], info["order_costs"], info["part_costs"]):
                if oc.count(min(oc)) > 1:
                    tie_order = True
                    assert o == oc.index(min(oc))                # the smallest order
                if pc.count(min(pc)) > 1:
                    tie_part = True
                    assert p == pc.index(min(pc))                # the smallest partition order
            t = info["totals"]
            if t is not None and t.count(min(t)) > 1:
                tie_mode = True
                assert info["mode"] == S.MODES[t.index(min(t))]  # the earlier assignment
    assert orders == {0, 1, 2, 3, 4}
    assert porders == {0, 1, 2, 3, 4, 5, 6}
    assert modes == set(S.MODES)
    assert tie_order and tie_part and tie_mode
    # what the named cases are there for
    by = {c["name"]: restated(i)[3] for i, c in enumerate(CASES)}
    assert [by[k][0]["orders"] for k in ("white", "walk", "walk2")] == [[0], [1], [2]]
    assert [by["sine%d" % p][0]["orders"] for p in ORDER_SINES] == [[3], [4]]
    assert [by["step%d" % p][0]["porders"] for p in range(7)] == [[p] for p in range(7)]
    assert [by["stereo-" + k][0]["mode"] for k in S.MODES] == list(S.MODES)
    assert by["tie-assignment"][0]["mode"] == "left/side" and len(set(by["tie-assignment"][0]["totals"][1:])) == 1
    assert by["silence-order-0"][0]["orders"] == [0]
    # the lengths: below 16 is effort 0's frame; 16 has one partition; 1024 reaches 16-sample partitions; the short block of 1000 has pmax 3
    assert [S.pmax(n) for n in (16, 17, 32, 1000, 1024, 4096)] == [0, 0, 1, 3, 6, 6]
    assert by["random-15-2ch"][0]["mode"] is None and by["sine-4095-2ch"] == []


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_host_effort_1_equals_the_restatement(engine_lib, i):
    c = CASES[i]
    want, sizes, used, _ = restated(i)
    got, res, consumed = host(engine_lib, c, 1)
    assert got == want
    assert (res.bytes_out, res.min_frame_bytes, res.max_frame_bytes) == (sum(sizes), min(sizes, default=0), max(sizes, default=0))
    assert consumed == used


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_effort_1_decodes_to_the_input_and_is_never_longer(engine_lib, i):
    c = CASES[i]
    s = c["samples"]
    got, _, consumed = host(engine_lib, c, 1)
    back, sizes, infos = S.decode(got, s.shape[1], c["depth"], first_block=c["first_block"])      # (asserts every CRC-8 and CRC-16)
    assert np.array_equal(back, s[:consumed])
    # the decoder read the choices the restatement made
    for seen, f in zip(infos, restated(i)[3]):
        if f["mode"]:
            assert seen == (S.MODE_NIBBLE.get(f["mode"], s.shape[1] - 1), list(zip(f["orders"], f["porders"])))
    # frame for frame no longer than effort 0
    plain = R.encode(s, c["depth"], first_block=c["first_block"], final=c["final"])[1]
    assert len(sizes) == len(plain) and all(a <= b for a, b in zip(sizes, plain))


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_effort_0_through_the_new_entry_is_the_old_entry(engine_lib, i):
    c = CASES[i]
    s = c["samples"]
    ch, frames = s.shape[1], s.shape[0]
    L = engine_lib.lib()
    pcm = R.pack_pcm(s, c["depth"])
    cap = engine_lib.flac_bound_bytes(ch, c["depth"], frames, c["final"])
    out = np.zeros(max(cap, 1), dtype=np.uint8)
    res, used = engine_lib.FlacResult(), C.c_size_t()
    assert L.d2d_flac_encode_host(ch, c["depth"], pcm.ctypes.data, frames, c["first_block"], int(c["final"]), out.ctypes.data, cap,
                                  C.byref(res), C.byref(used)) == 0
    got, res1, consumed = host(engine_lib, c, 0)
    assert got == out[:res.bytes_out].tobytes() == R.encode(s, c["depth"], first_block=c["first_block"], final=c["final"])[0]
    assert (res1.bytes_out, res1.min_frame_bytes, res1.max_frame_bytes, consumed) == (res.bytes_out, res.min_frame_bytes, res.max_frame_bytes, used.value)


def test_an_unknown_effort_is_refused_with_nothing_written(engine_lib):
    L = engine_lib.lib()
    s = R.signal("sine", BLOCK + 10, 2, 24)
    pcm = R.pack_pcm(s, 24)
    cap = engine_lib.flac_bound_bytes(2, 24, BLOCK + 10, 1)
    for effort in (2, 7, 0xFFFFFFFF):
        out = np.full(cap, 0xA5, dtype=np.uint8)
        res, used = engine_lib.FlacResult(111, 222, 333), C.c_size_t(444)
        rc = L.d2d_flac_encode_host_effort(2, 24, effort, pcm.ctypes.data, BLOCK + 10, 0, 1, out.ctypes.data, cap, C.byref(res), C.byref(used))
        assert rc == -1 and b"effort" in L.d2d_flac_error()
        assert (out == 0xA5).all() and (res.bytes_out, res.min_frame_bytes, res.max_frame_bytes, used.value) == (111, 222, 333, 444)
        # the device entry and the stream driver answer on the host, before any device call: these pointers are never dereferenced
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
