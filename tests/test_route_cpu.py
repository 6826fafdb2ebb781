"""Which kernel, table layout, staging and launch serve an engine: dsd2dxd_amd/csrc/d2d_route.cpp on the CPU, pinned by goldens.

tools/route_probe.cpp is built from that unit and d2d_tables.cpp with g++ alone.  Both goldens were recorded from the commit before the route
moved into one unit (profiles/route_refactor_check.md), so a condition that changes shows here, next to its cause, and not as a slower kernel
that a GPU parity test happens to name:
  tests/golden/route_predicates.json   the lookups and predicates (`route_probe predicates`, linked against that commit's library; the LDS
                                       sizes and mfma2_pipelined as one digest per filter and debug value: predicate_blocks)
  tests/golden/route_matrix.json       what an MI355X reported for every configuration of tools/engine_matrix.py (tools/route_matrix.py);
                                       tests/test_gpu_route.py holds an engine per outcome to it on the GPU
  tests/golden/route_fields.json       every other field the probe prints for those configurations (il2, coop, deinterleave, B, keep,
                                       mfma_pipe_lo, mono2_pipe, the launch geometry, the fp6 unit), one digest per rate and filter.  The
                                       parent had no place to read them from, so this one was recorded from the moved code, once its
                                       engine_matrix output had compared equal to the parent's on the GPU: it pins what is, for later changes
  tests/golden/route_launches.json     the launch plans of those configurations (`route_probe launches -`: family, unit, LDS bytes, waves, tile,
                                       rows per file and kernel name of every pass), one digest per rate and filter; recorded from the code that
                                       first had plans, once its engine_matrix output had compared equal to its parent's on the GPU
                                       (profiles/launch_plan_check.md): a pin for later changes too
Where the name predicted before the first call differs from the kernel that was then launched, the golden keeps both; this test asserts the
prediction against route_kernel_name (d2d_kernel_name's text moved unchanged) and the launched name against the plan's."""
import hashlib
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from route_matrix import expand, key, load  # noqa: E402
from test_gpu_parity import RATE_MATRIX  # noqa: E402


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("route_probe") / "route_probe")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    csrc = os.path.join("..", "dsd2dxd_amd", "csrc")
    cmd = ["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"),
           "-o", exe, "route_probe.cpp", os.path.join(csrc, "d2d_route.cpp"), os.path.join(csrc, "d2d_tables.cpp")]
    r = subprocess.run(cmd, cwd=os.path.join(ROOT, "tools"), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return exe


def _run(exe, *args, stdin=None):
    p = subprocess.run([exe, *args], input=stdin, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout[-500:], p.stderr[-500:])
    return p.stdout.strip().split("\n")


@pytest.fixture(scope="module")
def matrix():
    """the golden's groups, each group's terms expanded to its keys"""
    groups = load(os.path.join(ROOT, "tests", "golden", "route_matrix.json"))
    return [dict(g, configurations=[k for t in g["configurations"] for k in expand(t)]) for g in groups]


@pytest.fixture(scope="module")
def routes(probe, matrix):
    """key -> the rest of the probe's line, for every configuration of the golden"""
    keys = [k for g in matrix for k in g["configurations"]]
    lines = [l.split("\t", 1) for l in _run(probe, "-", stdin="\n".join(keys) + "\n")]
    assert [k for k, _ in lines] == keys
    return dict(lines)


@pytest.fixture(scope="module")
def launches(probe, matrix):
    """key -> the rest of the probe's `launches` line, for every configuration of the golden"""
    keys = [k for g in matrix for k in g["configurations"]]
    lines = [l.split("\t", 1) for l in _run(probe, "launches", "-", stdin="\n".join(keys) + "\n")]
    assert [k for k, _ in lines] == keys
    return dict(lines)


def _digests(lines_by_key):
    """the probe's lines as one "<lines> <first 16 hex digits of their sha256>" per rate and filter"""
    blocks = {}
    for k, rest in lines_by_key.items():
        blocks.setdefault(":".join(k.split(":")[:3]), []).append(k + "\t" + rest)
    return {k: "%d %s" % (len(b), hashlib.sha256("\n".join(b).encode()).hexdigest()[:16]) for k, b in blocks.items()}


def _fields(rest):
    head, name = rest.split(" name=")                  # (the name holds blanks and comes last)
    return dict([kv.split("=", 1) for kv in head.split(" ")], name=name)


def predicate_blocks(lines):
    """The probe's predicate lines as the golden holds them: shape/ and poly/ lines as they are, the smem/ lines of a filter and the pipe/
    lines of a (filter, debug value) as "<lines> <first 16 hex digits of the sha256 of those lines>"."""
    out, blocks = {}, {}
    for l in lines:
        k, v = l.split(" ", 1)
        part = k.split("/")
        if part[0] in ("shape", "poly"):
            assert k not in out
            out[k] = v
        else:
            blocks.setdefault("/".join(part[:2] + part[4:]), []).append(l)
    for k, b in blocks.items():
        assert len(set(b)) == len(b)
        out[k] = "%d %s" % (len(b), hashlib.sha256("\n".join(b).encode()).hexdigest()[:16])
    return out


def test_every_predicate_equals_the_golden(probe):
    probed = predicate_blocks(_run(probe, "predicates"))
    with open(os.path.join(ROOT, "tests", "golden", "route_predicates.json")) as f:
        golden = json.load(f)
    assert probed == golden, [(k, probed.get(k), golden.get(k)) for k in sorted(set(probed) | set(golden)) if probed.get(k) != golden.get(k)][:5]


def test_the_matrix_golden_holds_the_whole_sweep(matrix):
    """every configuration of tools/engine_matrix.py in exactly one outcome group"""
    from engine_matrix import configurations
    keys = [k for g in matrix for k in g["configurations"]]
    assert len(keys) == len(set(keys))
    assert set(keys) == {key(cfg) for cfg in configurations()}
    assert len({json.dumps(g["outcome"], sort_keys=True) for g in matrix}) == len(matrix)


def test_the_sweep_covers_the_rate_matrix(routes):
    assert {tuple(k.split(":")[:3]) for k in routes} == {(str(d), str(o), f) for d, o, f in RATE_MATRIX}


def test_every_route_equals_what_the_gpu_reported(routes, matrix):
    """create error (code and text), the predicted kernel name, the kernel and the table variant of every configuration of the sweep"""
    bad = []
    for g in matrix:
        want = g["outcome"]
        for k in g["configurations"]:
            rest = routes[k]
            if "create_error" in want:
                code, text = want["create_error"]
                ok = rest == "error=%d:%s" % (code, text)
            else:
                got = _fields(rest)
                ok = (got["name"] == want["kernel_name"] and int(got["kernel"]) == want["info"]["kernel"] and
                      got["table_variant"] == got["variant"])           # (choose_route's field and route_table_variant)
                if want["header"]:                                       # (two-pass 32-bit taps export no blob)
                    ok = ok and int(got["kernel"]) == want["header"]["kernel"] and int(got["table_variant"]) == want["header"]["table_variant"]
            if not ok:
                bad.append((k, rest, want))
    assert not bad, (len(bad), bad[:3])


def test_every_route_field_equals_the_golden(routes):
    """the whole line of every configuration of the sweep, staging and launch geometry included, as one digest per rate and filter"""
    probed = _digests(routes)
    with open(os.path.join(ROOT, "tests", "golden", "route_fields.json")) as f:
        golden = json.load(f)
    assert probed == golden, [(k, probed.get(k), golden.get(k)) for k in sorted(set(probed) | set(golden)) if probed.get(k) != golden.get(k)]


def test_every_launch_plan_names_the_kernel_the_gpu_launched(routes, launches, matrix):
    """kernel_name_after of every creatable configuration of the sweep is the name of the plan its call took: the mono pair's where the engine has
    one, else the main pass's.  The sweep's one call feeds a fresh engine 8192 bytes per channel.  plan_call (d2d_engine.cpp) sends it through
    the pair when the halves (4096 bytes) are whole 16-byte chunks, whole outputs (M / 8 is 1, 2, 4, 8 or 16 bytes per output), no shorter than
    the history `keep`, and the outputs (8192 / (M / 8)) are even in number and end below 2^32: all but `keep` hold by arithmetic, `keep` is
    asserted here."""
    bad, creatable = [], 0
    for g in matrix:
        if "create_error" in g["outcome"]:
            continue
        for k in g["configurations"]:
            creatable += 1
            status, *passes = launches[k].split("\t")
            plans = {p.split(" ", 1)[0]: _fields(p.split(" ", 1)[1]) for p in passes}
            assert status == "ok" and "main" in plans, (k, launches[k])
            got = _fields(routes[k])
            assert ("m2" in plans) == (got["mono2_pipe"] != "0") and ("lo" in plans) == (got["fine"] == "1"), (k, launches[k])
            if "m2" in plans:
                assert int(got["keep"]) <= 4096, (k, got["keep"])
            plan = plans["m2" if "m2" in plans else "main"]
            if plan["name"] != g["outcome"]["kernel_name_after"] or int(plan["unit"]) < 0:
                bad.append((k, plan, g["outcome"]["kernel_name_after"]))
    assert creatable == 16720
    assert not bad, (len(bad), bad[:3])


def test_every_launch_plan_equals_the_golden(launches):
    """family, unit, LDS bytes, waves, tile, rows per file and name of every pass of every configuration of the sweep"""
    probed = _digests(launches)
    with open(os.path.join(ROOT, "tests", "golden", "route_launches.json")) as f:
        golden = json.load(f)
    assert probed == golden, [(k, probed.get(k), golden.get(k)) for k in sorted(set(probed) | set(golden)) if probed.get(k) != golden.get(k)]
