"""Every operand table the kernels read, built on the host by dsd2dxd_amd/csrc/d2d_tables.cpp and pinned byte for byte.

tools/table_probe.cpp is built from that unit with g++ alone and prints one line per table (key, bytes, 64-bit FNV-1a of the bytes), the
exactness predicates that gate kernel choice and the sums.  tests/golden/table_digests.json holds those lines as they were recorded
before the builders were gathered into one unit (profiles/tables_refactor_check.md): a builder that changes a byte fails here, next to
its cause, not in a GPU parity test.  tests/test_gpu_tables.py shows that an engine uploads what the builders built."""
import json
import os
import subprocess

import pytest

import adversarial as A
from test_extreme_sums_cpu import _headroom, _one_pass

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "table_digests.json")
KINDS = ("lut", "one_group", "two_group", "pipelined", "fp6", "fp6_wide")


@pytest.fixture(scope="module")
def probed(tmp_path_factory):
    """key -> the rest of the probe's line"""
    exe = str(tmp_path_factory.mktemp("table_probe") / "table_probe")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    cmd = ["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"),
           "-o", exe, "table_probe.cpp", os.path.join("..", "dsd2dxd_amd", "csrc", "d2d_tables.cpp")]
    r = subprocess.run(cmd, cwd=os.path.join(ROOT, "tools"), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, (p.stdout[-500:], p.stderr[-500:])
    lines = [l.split(" ", 1) for l in p.stdout.strip().split("\n")]
    out = dict(lines)
    assert len(out) == len(lines)                      # no key twice
    return out


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_every_line_equals_the_golden(probed, golden):
    assert set(probed) == set(golden)                  # a table that vanishes from the enumeration fails, and so does a new one without a pin
    bad = [(k, probed[k], golden[k]) for k in sorted(golden) if probed[k] != golden[k]]
    assert not bad, bad[:5]


def test_the_enumeration_is_complete(probed):
    """all 16 filters and the residual of each (every one has half32), both bit orders, every kind; all 8 composed tables, all 3 resamplers;
    a builder that is not defined for a filter shows as n/a and not as a missing key"""
    T = A.tables()
    want = set()
    for name, t in T["filters"].items():
        assert "q32" in t
        for n in (name, name + ".residual"):
            want |= {"%s/%s/%s" % (n, o, k) for o in "LM" for k in KINDS} | {"%s/%s" % (n, v) for v in ("mx_exact", "mx_wide_exact", "sum_abs_q")}
            for o in "LM":
                assert (probed["%s/%s/fp6" % (n, o)] == "n/a") == (t["M"] < 32)
                assert (probed["%s/%s/fp6_wide" % (n, o)] == "n/a") == (t["M"] < 32 or probed[n + "/mx_wide_exact"] == "0")
    for name in T["polys"]:
        want |= {"%s/%s" % (name, v) for v in ("px", "px_exact", "max_phase_sum_abs")}
    with open(os.path.join(ROOT, "filters", "filter_tables.json")) as f:
        resamplers = [r["name"] for r in json.load(f)["resamplers"]]
    for name in resamplers:
        want |= {"%s/%s" % (name, v) for v in ("resamp2", "nstep")}
    assert len(T["filters"]) == 16 and len(T["polys"]) == 8 and len(resamplers) == 3
    assert set(probed) == want


def test_the_two_bit_orders_of_every_table_differ(probed):
    """a control that the keys are not degenerate: the same bytes under both orders would mean the order never reached the builder"""
    n = 0
    for k, v in probed.items():
        if "/L/" in k and v != "n/a":
            assert v != probed[k.replace("/L/", "/M/")], k
            assert v.split()[0] == probed[k.replace("/L/", "/M/")].split()[0], k       # ... at equal size
            n += 1
    assert n == 2 * 16 * 4 + 2 * 8 + 7         # four int8 / LUT kinds of 16 filters and residuals, fp6 at M >= 32 (8 filters), seven digits (all of those but E_M128)


def test_sum_abs_q_is_the_headroom_tables(probed):
    """sum|q| 2^-S of every 24-bit filter against tests/test_extreme_sums_cpu.py::test_headroom_table's |v| / 2^S, derived there from
    filters/filter_tables.json in Python integers"""
    for name in A.tables()["filters"]:
        g, S, M = A.fir_taps(name)
        assert int(probed[name + "/sum_abs_q"]) / 2.0 ** S == _headroom(g, S, M)["v"][0] / 2.0 ** S, name
        assert int(probed[name + "/sum_abs_q"]) == _headroom(g, S, M)["v"][0]
    for name in A.POLYS:
        q2, t = A.poly_taps(name)
        assert int(probed[name + "/max_phase_sum_abs"]) == max(_headroom(q2[rho], t["S"])["v"][0] for rho in range(t["Lp"])), name


def test_the_predicates_hold_where_the_kernels_rely_on_them(probed):
    """px_exact for all eight composed tables; mx_exact for every filter of DESIGN section 4.0's headroom table (all sixteen: the table bounds
    the five-digit parts of each), mx_wide_exact for the two the one-pass route serves"""
    for name in A.POLYS:
        assert probed[name + "/px_exact"] == "1", name
    for name in A.tables()["filters"]:
        assert probed[name + "/mx_exact"] == "1", name
        if _one_pass(name):
            assert probed[name + "/mx_wide_exact"] == "1", name
    assert probed["E_M128/mx_wide_exact"] == "0"       # (its bound is over 2^24: that table runs in two passes)
