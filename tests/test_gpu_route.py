"""An engine takes the route tests/golden/route_matrix.json recorded: one configuration per distinct outcome of the sweep of
tools/engine_matrix.py, created and run over two 4096-byte blocks per channel exactly as the sweep does it.  kernel_name() before and after
the call, info() and the exported blob's header (kernel, table_variant, fir_bytes) equal the golden; no kernel name is asserted beyond what
the golden recorded.  tests/test_route_cpu.py holds every configuration of the sweep to the same file on the CPU."""
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from route_matrix import expand, key, load, outcome  # noqa: E402

GROUPS = load(os.path.join(ROOT, "tests", "golden", "route_matrix.json"))
FIRST = [expand(g["configurations"][0])[0] for g in GROUPS]


@pytest.fixture(scope="module")
def sweep(engine_lib):
    """the first configuration of every outcome group, and the sweep's call buffer"""
    from engine_matrix import call_buffer, configurations
    first = {k: i for i, k in enumerate(FIRST)}
    cfgs = {first[key(cfg)]: cfg for cfg in configurations() if key(cfg) in first}
    assert len(cfgs) == len(GROUPS)
    return cfgs, call_buffer()


@pytest.mark.parametrize("group", range(len(GROUPS)), ids=FIRST)
def test_engine_takes_the_recorded_route(sweep, group):
    from engine_matrix import describe
    cfgs, data = sweep
    assert outcome(describe(cfgs[group], data)) == GROUPS[group]["outcome"]
