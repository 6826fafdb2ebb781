"""tests/golden/kernel_instances.json is the list of FIR kernel instantiations the route can reach, one configuration each, as
tools/kernel_instances.py derives it from tools/route_probe.cpp's full sweep: regenerated here and compared in both directions.

tests/test_gpu_kernel_instances.py converts every row of the file on the GPU against the oracle, so the file is the statement of which
instantiations that comparison reaches.  A new row of D2D_MX_UNIT_LIST / D2D_M3_UNIT_LIST / D2D_PX_UNIT_LIST or a new condition in
d2d_route.cpp that the sweep reaches makes a unit the file lacks; a condition that moves makes a row whose key no longer reaches its kernel.
Both fail here until `python tools/kernel_instances.py` has written the file again, and the GPU file then has a case for the new unit."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import kernel_instances as K  # noqa: E402
from route_matrix import load  # noqa: E402


@pytest.fixture(scope="module")
def golden():
    with open(K.GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def generated(tmp_path_factory):
    return K.generate(K.build_probe(str(tmp_path_factory.mktemp("route_probe") / "route_probe")))


def _by_unit(rows):
    out = {K.unit_id(r): r for r in rows}
    assert len(out) == len(rows)                         # (an id names one unit)
    return out


def test_the_golden_is_the_generated_unit_list(golden, generated):
    got, want = _by_unit(generated), _by_unit(golden)
    assert sorted(set(got) - set(want)) == [], "units without a case: run tools/kernel_instances.py"
    assert sorted(set(want) - set(got)) == [], "cases whose unit the sweep no longer has: run tools/kernel_instances.py"
    moved = [(u, got[u], want[u]) for u in want if got[u] != want[u]]
    assert not moved, (len(moved), moved[:3])
    assert generated == golden                           # (and in the file's order)
    with open(K.GOLDEN) as f:
        assert f.read() == K.dumps(generated)


def test_every_row_names_its_unit_in_its_own_plans(golden):
    """what the GPU file relies on: the unit's kernel is the plan of the unit's pass, `lo` units are fine routes, `m2` units have a pair"""
    for r in golden:
        u = r["unit"]
        assert r["passes"][u["pass"]]["name"] == u["name"], r
        assert r["pair"] == ("m2" in r["passes"]) and (r["fine"] == 1) == ("lo" in r["passes"]), r
        assert (u["depth"] is None) == (r["family"] not in K.RUNTIME_EPILOGUE and not u["scratch"]), r
        assert u["depth"] in (None, K.parse_key(r["key"])["bit_depth"]), r
        assert (u["form"] is not None) == (r["family"] == "px"), r


def test_the_gpu_file_names_the_units_as_the_tool_does(golden):
    import test_gpu_kernel_instances as T
    assert T.ROWS == golden and [T.unit_id(r) for r in golden] == [K.unit_id(r) for r in golden]
    assert [T.parse_key(r["key"]) for r in golden] == [K.parse_key(r["key"]) for r in golden]


def test_the_runtime_epilogue_families_meet_every_dither_and_both_levels(golden):
    for fam in K.RUNTIME_EPILOGUE:
        cfgs = [K.parse_key(r["key"]) for r in golden if r["family"] == fam]
        assert {c["dither"] for c in cfgs} == set(K.DITHERS) and {c["level_db"] for c in cfgs} == set(K.LEVELS), fam


def test_the_units_hold_every_kernel_the_route_golden_recorded(golden):
    """the kernel_name_after values of tests/golden/route_matrix.json (what an MI355X launched over tools/engine_matrix.py's sweep)"""
    after = {g["outcome"]["kernel_name_after"] for g in load(os.path.join(ROOT, "tests", "golden", "route_matrix.json")) if "create_error" not in g["outcome"]}
    names = {r["unit"]["name"] for r in golden}
    assert len(after) == 200 and after <= names, sorted(after - names)
    assert len(names) >= 347
