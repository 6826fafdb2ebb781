"""The inputs of tests/test_gpu_flac_edges.py, and the proof that they are what that file needs them to be.  The GPU tests compare the
device with d2d_flac_encode_host; here the host encoder is pinned to the plain-Python restatement (flac_ref.encode) on every one of those
inputs, and the conditions the inputs were chosen for are asserted from the restatement's own arithmetic: every Rice parameter is
reached, the tuned sums put k on each side of its threshold, the spikes give the unary runs they are there for, and the pack kernel's
workgroups start at every byte alignment.  No GPU."""
import functools

import numpy as np
import pytest

import flac_ref as R

B = R.BLOCK
DEPTHS = (16, 20, 24)


def check_host(engine_lib, samples, depth, first_block=0, final=True):
    """host == restatement, the record, frames consumed, every frame within the bound; returns the frame sizes"""
    samples = np.asarray(samples, dtype=np.int64)
    frames, ch = samples.shape
    want, sizes, used = R.encode(samples, depth, first_block=first_block, final=final)
    got, res, consumed = engine_lib.flac_encode_host(ch, depth, R.pack_pcm(samples, depth), first_block=first_block, final=final)
    assert got == want
    assert (res.bytes_out, res.min_frame_bytes, res.max_frame_bytes) == (sum(sizes), min(sizes, default=0), max(sizes, default=0))
    assert consumed == used
    for i, fs in enumerate(sizes):
        assert fs <= R.frame_bound(ch, depth, min(B, frames - B * i)), i
    return sizes


def block_stats(samples):
    """[(k, longest unary run)] of every (block, channel) of a final file"""
    s = np.asarray(samples, dtype=np.int64)
    return [R.rice_stats(s[b:b + B, c]) for b in range(0, s.shape[0], B) for c in range(s.shape[1])]


# ---- K_SWEEP: every Rice parameter -----------------------------------------------------------------------------------------------
# Stereo noise at every amplitude step 2^0 .. 2^(depth-1), two blocks (the second short and odd).  From 2^3 on a step of the amplitude is a step of k (2^a gives
# k = a + 1), but at the bottom the whole steps skip a value -- 2^1 gives k = 1 and 2^2 gives k = 3, bar one short block that happens
# to get 2 -- so the half step 2^1.5, which gives k = 2 in every block, is in the list.  "alternate" gives the largest k: depth + 1.
K_FRAMES = B + 259
K_SWEEP = tuple((d, "noise", a) for d in DEPTHS for a in list(range(d)) + [1.5]) + tuple((d, "alternate", None) for d in DEPTHS)
K_TOP = {16: 17, 20: 21, 24: 25}


@functools.lru_cache(maxsize=None)
def k_sweep_signal(depth, kind, amp_bits):
    if kind == "alternate":
        return R.signal("alternate", K_FRAMES, 2, depth)
    return R.noise(K_FRAMES, 2, depth, amp_bits, seed=int(10 * amp_bits) + depth)


@pytest.mark.parametrize("depth", DEPTHS)
def test_k_sweep_reaches_every_rice_parameter(engine_lib, depth):
    reached = set()
    for d, kind, a in K_SWEEP:
        if d != depth:
            continue
        s = k_sweep_signal(d, kind, a)
        check_host(engine_lib, s, d)
        reached |= {k for k, _ in block_stats(s)}
    assert R.rice_stats(R.signal("alternate", B, 1, depth)[:, 0])[0] == K_TOP[depth]
    assert reached == set(range(K_TOP[depth] + 1)), sorted(set(range(K_TOP[depth] + 1)) - reached)


# ---- K_EDGES: a mean of exactly 2^j, of just under 2^j + 1, and of 2^j + 1 -----------------------------------------------------------
# One file per (n, depth, j), its three channels the three tuned sums: k = (j, j, j + 1).  The device adds |r| in another order than the
# host; a sum that is one off moves k only here.
K_EDGE_N = (259, B)
K_EDGE_J = (0, 1, 2, 5, 9, 12)
K_EDGES = tuple((n, d, j) for n in K_EDGE_N for d in (16, 24) for j in K_EDGE_J)


def k_edge_targets(n, j):
    return ((1 << j) * (n - 2), ((1 << j) + 1) * (n - 2) - 1, ((1 << j) + 1) * (n - 2))


@functools.lru_cache(maxsize=None)
def k_edge_signal(n, depth, j):
    return np.stack([R.tuned_sum(depth, n, t, seed=100 * j + i) for i, t in enumerate(k_edge_targets(n, j))], axis=1)


@pytest.mark.parametrize("n,depth,j", K_EDGES)
def test_k_edges_sit_on_both_sides_of_the_threshold(engine_lib, n, depth, j):
    s = k_edge_signal(n, depth, j)
    for c, t in enumerate(k_edge_targets(n, j)):
        assert int(np.abs(R.residuals(s[:, c])).sum()) == t
    assert [k for k, _ in block_stats(s)] == [j, j, j + 1]         # (the second and the third sum differ by one)
    check_host(engine_lib, s, depth)


# ---- SPIKES: where the outlier sits ------------------------------------------------------------------------------------------------
# (frames, index): a full block with the spike in its warm-up samples, in the first residuals, around a wave boundary (thread 64 owns
# samples 256 .. 259) and in the last thread's quartet; a short odd block with the spike in its last two samples.  Full scale (a unary
# run that crosses many threads' bits) and 40 (in silence: k = 0 and a run of 160 bits), in silence and over +/- 1 noise.
SPIKE_SHORT = 1001
SPIKE_AT = tuple((B, i) for i in (0, 1, 2, 3, 4, 5, 255, 256, 257, 4092, 4093, 4094, 4095)) + ((SPIKE_SHORT, SPIKE_SHORT - 2), (SPIKE_SHORT, SPIKE_SHORT - 1))
SPIKES = tuple((d, frames, i, amp, floor) for d in (16, 24) for frames, i in SPIKE_AT for amp in ("full", 40) for floor in (0, 1))


@functools.lru_cache(maxsize=None)
def spike_signal(depth, frames, index, amp, floor):
    return R.spike_at(frames, 2, depth, index, (1 << (depth - 1)) - 1 if amp == "full" else amp, floor)


def test_spikes_give_the_runs_they_are_there_for(engine_lib):
    longest, longest_k0 = 0, 0
    for d, frames, i, amp, floor in SPIKES:
        s = spike_signal(d, frames, i, amp, floor)
        assert s[i, 0] == -s[i, 1] != 0
        check_host(engine_lib, s, d)
        for k, run in block_stats(s):
            longest = max(longest, run)
            if k == 0:
                longest_k0 = max(longest_k0, run)
    assert longest > 4096, longest               # a run that crosses the bits of many threads
    assert longest_k0 > 32, longest_k0           # k = 0: the stop bit alone is written, more than a word behind the code's start


# ---- SHORT_N: last blocks of every residue mod 4 -------------------------------------------------------------------------------------
SHORT_N = (4, 5, 6, 7, 8, 63, 64, 65, 255, 257, 1023, 4093, 4094, 4095)
SHORT_SHAPES = ((1, 16), (2, 24), (3, 24), (5, 20), (7, 16))
SHORT_FILES = tuple((lead, n) for n in SHORT_N for lead in (0, B))          # (frames in front of the short block, the short block)


@functools.lru_cache(maxsize=None)
def short_signal(channels, depth, lead, n):
    return R.signal("random", lead + n, channels, depth, seed=n + lead + channels)


@pytest.mark.parametrize("channels,depth", SHORT_SHAPES)
def test_short_last_blocks(engine_lib, channels, depth):
    for lead, n in SHORT_FILES:
        sizes = check_host(engine_lib, short_signal(channels, depth, lead, n), depth, first_block=3)
        assert len(sizes) == (2 if lead else 1)
    assert {n % 4 for n in SHORT_N} == {0, 1, 2, 3}


# ---- MANY_BLOCKS: more than one pack workgroup (32 blocks each), more sizes than one pass of its reduction (256) ------------------------
# (channels, depth, full blocks, tail, first_block, final): mono 16-bit files of 31 .. 300 blocks, some with a short last block, one
# whose frame numbers pass 0x7FF -> 0x800 inside it, a 33-block stereo 24-bit file, a 1-block and a 0-block file
MANY_BLOCKS = ((1, 16, 31, 0, 0, True), (1, 16, 32, 0, 0, True), (1, 16, 32, 1000, 5, True), (1, 16, 64, 0, 0x7F0, True),
               (1, 16, 64, 5, 0, True), (1, 16, 288, 0, 0, True), (1, 16, 288, 4093, 0, True), (1, 16, 300, 0, 0, True),
               (1, 16, 1, 0, 9, True), (1, 16, 0, 100, 0, False),
               (2, 24, 32, 77, 0, True))


def many_blocks_count(spec):
    _, _, full, tail, _, final = spec
    return full + (1 if final and tail else 0)


@functools.lru_cache(maxsize=None)
def many_blocks_signal(spec):
    ch, depth, full, tail, _, _ = spec
    return R.varying(full * B + tail, ch, depth, seed=full + tail)


@functools.lru_cache(maxsize=None)
def _many_blocks_sizes(engine_lib, spec):
    return tuple(check_host(engine_lib, many_blocks_signal(spec), spec[1], first_block=spec[4], final=spec[5]))


@pytest.mark.parametrize("spec", MANY_BLOCKS, ids=lambda s: f"{s[0]}ch{s[1]}-{s[2]}x4096+{s[3]}")
def test_many_blocks(engine_lib, spec):
    sizes = _many_blocks_sizes(engine_lib, spec)
    assert len(sizes) == many_blocks_count(spec)
    if len(sizes) > 1:
        assert max(sizes) >= 2 * min(sizes)                            # the frames of one file differ in size


def test_many_blocks_cover_what_the_pack_kernel_branches_on(engine_lib):
    counts = sorted(many_blocks_count(s) for s in MANY_BLOCKS if s[:2] == (1, 16))
    assert counts == [0, 1, 31, 32, 33, 64, 65, 288, 289, 300]
    starts = set()
    for spec in MANY_BLOCKS:
        off = np.concatenate([[0], np.cumsum(_many_blocks_sizes(engine_lib, spec))])
        starts |= {int(off[b]) % 4 for b in range(32, many_blocks_count(spec), 32)}
    assert starts == {0, 1, 2, 3}, starts                              # byte offsets at which a later pack workgroup begins
    spec = next(s for s in MANY_BLOCKS if s[4] == 0x7F0)
    assert len(R.utf8_number(spec[4])) == 2 and len(R.utf8_number(spec[4] + many_blocks_count(spec) - 1)) == 3


# ---- decode round trip: a few blocks in all (the decoder is a per-sample Python loop) ---------------------------------------------------
ROUND_TRIP = {
    "k-edge": (lambda: k_edge_signal(259, 24, 9), 24),
    "k-edge-j0": (lambda: k_edge_signal(259, 16, 0), 16),
    "spike-last-sample": (lambda: spike_signal(24, SPIKE_SHORT, SPIKE_SHORT - 1, "full", 1), 24),
    "spike-k0": (lambda: spike_signal(16, SPIKE_SHORT, SPIKE_SHORT - 2, 40, 0), 16),
    "noise-half-step": (lambda: k_sweep_signal(16, "noise", 1.5)[B:], 16),
    "short-5": (lambda: short_signal(5, 20, 0, 5), 20),
    "short-7": (lambda: short_signal(5, 20, 0, 7), 20),
    "short-65": (lambda: short_signal(5, 20, 0, 65), 20),
    "short-4093": (lambda: short_signal(1, 16, 0, 4093), 16),
}


@pytest.mark.parametrize("what", ROUND_TRIP)
def test_decode_round_trip(engine_lib, what):
    make, depth = ROUND_TRIP[what]
    samples = make()
    got, _, _ = engine_lib.flac_encode_host(samples.shape[1], depth, R.pack_pcm(samples, depth), first_block=0, final=True)
    back, _ = R.decode(got, samples.shape[1], depth)              # (asserts every CRC-8 and CRC-16)
    assert np.array_equal(back, samples)
