"""ONE stream cut along time over N engine processes (BASELINE config 5's shape): every rank seeks to its
slice (dsd2dxd_amd.shard.shard_time), primes with the halo and converts; the concatenation of the ranks' frames is the single
engine's conversion and the oracle's, and every rank runs the single engine's kernel -- it keeps the whole stream's parameters."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _run_ranks(world, tmp_path):
    outs = [str(tmp_path / f"slice_{r}.npz") for r in range(world)]
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "timeslice_worker.py"), str(r), str(world), outs[r]],
                              stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for r in range(world)]      # (at most 3 at once)
    try:
        for p in procs:
            _, se = p.communicate(timeout=120)
            assert p.returncode == 0, se[-3000:]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    return [np.load(o) for o in outs]


_SINGLE = {}


def _single(engine_lib, oracle_mod):
    """the stream, the oracle's conversion and a single engine's: computed once for both worlds"""
    if not _SINGLE:
        import timeslice_worker as W
        from helpers import pack_layout
        buf = pack_layout(W.stream_channels(), "I", 1)
        o = oracle_mod.Oracle(**W.KW)
        want, fr = o.translate(buf)
        e = engine_lib.Engine(**W.KW)
        single, fr1 = e.translate(buf)
        assert fr1 == fr
        _SINGLE.update(want=want[:fr * o.frame_bytes].copy(), single=single.copy(), opeaks=[o.peak(c) for c in range(W.CHN)],
                       peaks=[e.peak(c) for c in range(W.CHN)], kernel=e.kernel_name())
        e.close()
    return _SINGLE


@pytest.mark.timeout(300)
@pytest.mark.parametrize("world", [2, 3])
def test_ranks_cut_one_stream_along_time(engine_lib, oracle_mod, tmp_path, world):
    import timeslice_worker as W
    from dsd2dxd_amd.shard import shard_range
    s = _single(engine_lib, oracle_mod)
    parts = _run_ranks(world, tmp_path)
    for r, part in enumerate(parts):
        halo, begin, end = (int(v) for v in part["range"])
        assert (begin, end) == shard_range(W.NBYTES, world, r) and 0 <= halo <= begin < end
        assert str(part["kernel"]) == s["kernel"], r
    assert all(int(p["range"][1]) - int(p["range"][0]) > 0 for p in parts[1:])          # every later rank had a halo to prime with
    cat = np.concatenate([p["pcm"] for p in parts])
    assert np.array_equal(cat, s["single"])
    assert np.array_equal(cat, s["want"])
    peaks = np.max(np.stack([p["peaks"] for p in parts]), axis=0)
    assert list(peaks) == s["peaks"] == s["opeaks"]
