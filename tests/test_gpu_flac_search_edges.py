"""flac_search_kernel<1..8, LPC or not> (dsd2dxd_amd/csrc/flac/d2d_flac.hip), FLAC efforts 1 and 12 on the GPU, at its edges and at
the integer bounds its comments state.  The inputs and the proof of what they reach are in tests/test_flac_search_edges_cpu.py:

  1. the edge corpora of the effort-0 kernel (tests/test_flac_edges_cpu.py: every Rice parameter and both sides of its thresholds,
     outliers at every alignment, last blocks of every residue mod 4, files of 300 blocks) through both efforts;
  2. EDGE_CASES: rail-level signals that attain |r| = 2^28 - 16 in the fixed residual sets, a 25-bit side signal, R(0) above 2^57,
     impulses and strongly resonant noise that make rule 13 drop candidates, every coefficient shift the rule can give;
  3. the verifier, at both methods, on what the device encoded from EDGE_CASES;
  4. d2dlpc::lpc_coefficients (flac_lpc.h) as hipcc builds it for the device, alone in a kernel (tools/flac_lpc_probe_gpu.hip), on
     autocorrelations that fire every one of its branches.

Every comparison is against d2d_flac_encode_host_effort -- which the CPU file pins to the Python restatements -- or against the
restatement itself, byte for byte.  test_gpu_flac_search.device_encode gives every file exactly its bound as capacity and asserts that
nothing behind bytes_out was written.  Up to 16 files share a call."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import flac_ref as R
import test_flac_edges_cpu as E
import test_flac_search_edges_cpu as X
from test_flac_verify_cpu import clean
from test_gpu_flac_coop import COOP, SERIAL, both_methods
from test_gpu_flac_search import device_encode, host_encode
from test_gpu_flac_verify import Batch

gpu = pytest.mark.gpu
B = R.BLOCK
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAXF = 16                                                          # files per launch (d2d_flac.hip)
EFFORTS = X.EFFORTS


def compare(d, channels, depth, effort, cases, per_call=MAXF, again=True):
    """cases: [(label, int64 samples (frames, channels), first_block, final)], `per_call` of them in each device call: frames, result
    record and frames_consumed are the host's; the same call once more gives the same bytes"""
    files = [(R.pack_pcm(s, depth), first, final) for _, s, first, final in cases]
    want = host_encode(d, channels, depth, files, effort=effort)
    for at in range(0, len(files), per_call):
        got = device_encode(d, channels, depth, files[at:at + per_call], effort=effort)
        for i, g in enumerate(got):
            label, w = cases[at + i][0], want[at + i]
            assert g[1] == w[1], label                             # the result record
            assert g[0] == w[0], label                             # the frames
            assert g[2] == w[2], label                             # frames_consumed
        if again:
            assert device_encode(d, channels, depth, files[at:at + per_call], effort=effort) == got
    return want


# ---- 1. the effort-0 edge corpora ------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("effort", EFFORTS)
@pytest.mark.parametrize("depth", E.DEPTHS)
def test_k_sweep(engine_lib, depth, effort):
    compare(engine_lib, 2, depth, effort, [(f"{kind} {a}", E.k_sweep_signal(d, kind, a), 0, True) for d, kind, a in E.K_SWEEP if d == depth])


@gpu
@pytest.mark.parametrize("effort", EFFORTS)
@pytest.mark.parametrize("depth", (16, 24))
def test_k_edges(engine_lib, depth, effort):
    compare(engine_lib, 3, depth, effort, [(f"n = {n}, j = {j}", E.k_edge_signal(n, d, j), 0, True) for n, d, j in E.K_EDGES if d == depth])


@gpu
@pytest.mark.parametrize("effort", EFFORTS)
@pytest.mark.parametrize("depth", (16, 24))
def test_spikes(engine_lib, depth, effort):
    compare(engine_lib, 2, depth, effort, [(f"{amp} at {i} of {frames}, floor {floor}", E.spike_signal(d, frames, i, amp, floor), 0, True)
                                           for d, frames, i, amp, floor in E.SPIKES if d == depth])


@gpu
@pytest.mark.parametrize("effort", EFFORTS)
@pytest.mark.parametrize("channels,depth", E.SHORT_SHAPES)
def test_short_last_blocks(engine_lib, channels, depth, effort):
    compare(engine_lib, channels, depth, effort, [(f"{lead} + {n}", E.short_signal(channels, depth, lead, n), 3, True) for lead, n in E.SHORT_FILES])


def _many(shape):
    return [(f"{s[2]} x 4096 + {s[3]}", E.many_blocks_signal(s), s[4], s[5]) for s in E.MANY_BLOCKS if s[:2] == shape]


def _blocks(frames, final):
    return frames // B + (1 if final and frames % B else 0)


@gpu
@pytest.mark.parametrize("effort", EFFORTS)
def test_many_blocks_share_a_call(engine_lib, effort):
    """files of 0, 1 and 31 .. 300 blocks in one call, as at effort 0: the grid is the largest file's"""
    cases = _many((1, 16))
    assert len(cases) == 10 and max(_blocks(s.shape[0], f) for _, s, _, f in cases) == 300
    want = compare(engine_lib, 1, 16, effort, cases)
    zero = [w for (_, s, _, f), w in zip(cases, want) if _blocks(s.shape[0], f) == 0]
    assert len(zero) == 1 and zero[0][1] == (0, 0, 0) and zero[0][0] == b""
    compare(engine_lib, 2, 24, effort, _many((2, 24)))


@gpu
@pytest.mark.parametrize("effort", EFFORTS)
def test_seventeen_files_reach_the_second_launch(engine_lib, effort):
    """one more file than a launch carries descriptors for: the spikes of one depth and a short last block behind them"""
    cases = [(f"{amp} at {i} of {frames}, floor {floor}", E.spike_signal(d, frames, i, amp, floor), 0, True)
             for d, frames, i, amp, floor in E.SPIKES if d == 24 and floor == 1][:16]
    cases.append(("the 17th", E.short_signal(2, 24, B, 4093), 3, True))
    assert len(cases) == 17
    compare(engine_lib, 2, 24, effort, cases, per_call=17)


# ---- 2. EDGE_CASES against the host, 3. the verifier on what the device made of them -----------------------------------------------------

def _group(channels, depth):
    return [c for c in X.EDGE_CASES if (c["samples"].shape[1], c["depth"]) == (channels, depth)]


@gpu
@pytest.mark.parametrize("effort", EFFORTS)
@pytest.mark.parametrize("channels,depth", X.EDGE_GROUPS, ids=lambda v: str(v))
def test_the_edge_cases_equal_the_host_encoder(engine_lib, channels, depth, effort):
    mine = _group(channels, depth)
    compare(engine_lib, channels, depth, effort, [(c["name"], c["samples"], c["first_block"], c["final"]) for c in mine])


@gpu
@pytest.mark.parametrize("effort", EFFORTS)
@pytest.mark.parametrize("channels,depth", X.EDGE_GROUPS, ids=lambda v: str(v))
def test_the_verifier_accepts_what_the_device_encoded(engine_lib, channels, depth, effort):
    """encode and both verify kernels on one batch; both_methods compares records and stats with the host twin's on the downloaded bytes"""
    mine = _group(channels, depth)
    for at in range(0, len(mine), MAXF):
        part = mine[at:at + MAXF]
        b = Batch(engine_lib, channels, depth, [(R.pack_pcm(c["samples"], depth), c["first_block"], c["final"]) for c in part])
        b.encode(effort)
        got = both_methods(b)
        want = [clean(io.frames_consumed, io.blocks) for io in b.ios]
        assert got[COOP][0] == want, [(c["name"], g) for c, g, w in zip(part, got[COOP][0], want) if g != w]
        assert got[COOP][1] == [(w[1], 0) for w in want] and got[SERIAL][1] == [(0, w[1]) for w in want]     # every block by the fast path
        for i, c in enumerate(part):                               # ... and what was verified is the host encoder's frame
            s = c["samples"]
            assert b.frames(i)[0].tobytes() == engine_lib.flac_encode_host(channels, depth, R.pack_pcm(s, depth), first_block=c["first_block"],
                                                                           final=c["final"], effort=effort)[0], c["name"]


# ---- 4. rule 13 on the device ----------------------------------------------------------------------------------------------------------

def _hipcc():
    return shutil.which("hipcc") or os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")


@pytest.fixture(scope="module")
def device_probe(tmp_path_factory):
    """tools/flac_lpc_probe_gpu.hip with the flags csrc/Makefile gives the kernels"""
    exe = str(tmp_path_factory.mktemp("flac_lpc_probe_gpu") / "flac_lpc_probe_gpu")
    r = subprocess.run([_hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-o", exe, "flac_lpc_probe_gpu.hip"],
                       cwd=os.path.join(ROOT, "tools"), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    return exe


@gpu
def test_the_device_routine_equals_the_host_routine_and_the_restatement(device_probe, tmp_path):
    """HAND, the autocorrelations of EDGE_CASES and the seeded set, one workgroup per vector, in a child process of its own"""
    vecs = X.vectors()
    got = X.run_probe(device_probe, vecs, tmp_path, timeout=120)
    X.assert_probe_equals_the_restatement(got)
    exe = os.path.join(str(tmp_path), "flac_lpc_probe")
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-o", exe, "flac_lpc_probe.cpp"], cwd=os.path.join(ROOT, "tools"),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert got == X.run_probe(exe, vecs, tmp_path, timeout=120)
