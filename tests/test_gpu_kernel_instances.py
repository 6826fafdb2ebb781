"""Every FIR kernel instantiation the route can reach, held to the oracle: one case per row of tests/golden/kernel_instances.json.

The file (tools/kernel_instances.py wrote it, tests/test_kernel_instances_cpu.py holds it to the route on the CPU) names for every coverage unit
-- a (pass, kernel) of the families whose name carries the sample format, a (pass, kernel, depth, scratch) of those whose epilogue is a runtime
argument, one per depth where the kernel writes the scratch, the composed polyphase kernel's by channel pair and single channel (two forms of its
tile loop under one name) -- one configuration that reaches it.  The engine is created from that key the way
tools/route_probe.cpp spells it (planar: blocks of 4096, LSB first; interleaved: bytes, MSB first; seed 7), the oracle with the same parameters
(filter 'S' is its cascade mode, tap_bits 32 its fine taps, which know float output under 'N' by the letter 'X' only), and both convert one stream in three calls.  With `tile`, `block_tiles` of the unit's
pass and b bytes per output (M / 8 of the FIR table; the rate ratio for the polyphase kernels):

  call 1   an even number of 4096-byte blocks per channel, at least 2 tile block_tiles + tile outputs: an interior tile between the careful edge
           tiles.  A mono engine with a pair takes the pair, which converts the two halves side by side: for an `m2` unit each half has that many.
  call 2   an odd number of bytes, about half a tile of outputs: a pair engine takes its ordinary kernel.
  call 3   an odd number of bytes, a tile and 37 outputs: history, dither index and peak carried across two call boundaries.  For the `main`
           unit of a pair engine, whose first call went to the pair, this call is as long as call 1's rule asks.

A channel is a seeded sine (even channels) or pink noise (odd) with a stretch of 0xFF and one of 0x00 in the long call, each longer than the
history the engine keeps (FIR window and stage B's): both rails at the integer depths.  After every call the frames, the bytes and every channel's
peak equal the oracle's; kernel_name() is the pair's after call 1 where there is one, the main pass's after every other call.  The residual pass of
a `lo` unit is not what kernel_name() reports: its row must be a fine route, whose every call runs it."""
import json
import os
from fractions import Fraction

import numpy as np
import pytest

from helpers import pack_layout, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "tests", "golden", "kernel_instances.json")) as _f:
    ROWS = json.load(_f)
RUNTIME_EPILOGUE = ("lut", "mfma", "mfma2", "px_plain")
POLYPHASE = ("px", "px_plain")
FIELDS = ("dsd_rate", "output_rate", "filter", "channels", "fmt", "bit_depth", "dither", "level_db", "tap_bits", "kernel", "debug")


def unit_id(row):
    u = row["unit"]
    return "%s:%s%s%s%s" % (u["pass"], u["name"].replace(" ", ""), "" if u["depth"] is None else ":%d" % u["depth"],
                            "s" if u["scratch"] and row["family"] in RUNTIME_EPILOGUE else "", ":" + u["form"] if u["form"] else "")


def parse_key(key):
    """<dsd_rate>:<output_rate>:<filter>:<channels><fmt><depth><dither>:<level>:<tap_bits>:<kernel>:<debug flags>"""
    dsd_rate, output_rate, filt, fmt, level, tap_bits, kernel, debug = key.split(":")
    i = min(fmt.index("P") if "P" in fmt else 99, fmt.index("I") if "I" in fmt else 99)
    return dict(zip(FIELDS, (int(dsd_rate), int(output_rate), filt, int(fmt[:i]), fmt[i], int(fmt[i + 1:-1]), fmt[-1], float(level), int(tap_bits),
                             int(kernel), int(debug))))


def call_sizes(row, cfg):
    """bytes per channel of the three calls, and the call that holds the rails"""
    plan = row["passes"][row["unit"]["pass"]]
    b = Fraction(cfg["dsd_rate"] * 352800, cfg["output_rate"]) if row["family"] in POLYPHASE else Fraction(row["M"], 8)
    tile, full = plan["tile"], 2 * plan["tile"] * plan["block_tiles"] + plan["tile"]
    ceil = lambda x: -(-x.numerator // x.denominator)
    n1 = 2 * full if row["unit"]["pass"] == "m2" else full
    c1 = -(-ceil(n1 * b) // 8192) * 8192
    c2 = ceil(tile * b) // 2 | 1
    main_of_pair = row["pair"] and row["unit"]["pass"] != "m2"
    c3 = ceil(((full if main_of_pair else tile) + 37) * b) | 1
    assert c2 % 16 and c3 % 16 and c1 % 8192 == 0
    return [c1, c2, c3], 2 if main_of_pair else 0


def stream(row, cfg, calls, rails_in):
    """the channels of the whole stream"""
    total = sum(calls)
    stretch = 2 * row["keep"] + 100 * (row["M"] // 8)       # (stage B of the cascade: 96 stage-A samples of M / 8 bytes)
    start, n = sum(calls[:rails_in]), calls[rails_in]
    assert 4 * stretch < n, (stretch, n)
    chans = []
    for c in range(cfg["channels"]):
        ch = synth("pink" if c % 2 else "sine", total, seed=11 + c, amp=0.098 if c % 2 else 0.352, freq=1000.0 + 111 * c, dsd_rate=cfg["dsd_rate"],
                   msb_first=cfg["fmt"] == "I")
        hi, lo = (1, 5) if c % 2 == 0 else (5, 1)            # (odd channels meet the rails in the other order, in the other half)
        ch[start + hi * n // 8:start + hi * n // 8 + stretch] = 0xFF
        ch[start + lo * n // 8:start + lo * n // 8 + stretch] = 0x00
        chans.append(ch)
    return chans


@pytest.mark.parametrize("row", ROWS, ids=[unit_id(r) for r in ROWS])
def test_unit_equals_the_oracle(engine_lib, oracle_mod, row):
    unit, cfg = row["unit"], parse_key(row["key"])
    assert row["passes"][unit["pass"]]["name"] == unit["name"]
    if unit["pass"] == "lo":
        assert row["fine"] == 1 and cfg["tap_bits"] == 32
    if unit["pass"] == "m2":
        assert row["pair"] and cfg["channels"] == 1
    if unit["form"]:
        assert cfg["channels"] >= 2 if unit["form"] == "pair" else cfg["channels"] % 2 == 1
    planar = cfg["fmt"] == "P"
    layout = dict(fmt=cfg["fmt"], endianness="L" if planar else "M", block_size=4096 if planar else 1, seed=7)
    common = {k: cfg[k] for k in ("dsd_rate", "output_rate", "channels", "bit_depth", "dither", "level_db")}
    e = engine_lib.Engine(filter=cfg["filter"], tap_bits=cfg["tap_bits"], kernel=cfg["kernel"], debug=cfg["debug"], **common, **layout)
    if cfg["tap_bits"] == 32 and cfg["bit_depth"] == 32 and cfg["dither"] == "N":
        # float output has nothing to shape: 'N' is 'X' to the engine (epilogue_of) and a plain cast to the oracle under either letter, but the
        # oracle's fine taps refuse the letter 'N'
        common = dict(common, dither="X")
    o = oracle_mod.Oracle(filter="E" if cfg["filter"] == "S" else cfg["filter"], tap_bits=cfg["tap_bits"] or 24, **common, **layout)
    if cfg["filter"] == "S":
        o.use_cascade()
    assert e.frame_bytes == o.frame_bytes
    # the plan counts the pass's own outputs: the frames, except in front of the cascade's stage B
    plan, exact = row["passes"][unit["pass"]], row["family"] in POLYPHASE or cfg["output_rate"] % 44100 == 0
    need = (2 if unit["pass"] == "m2" else 1) * (2 * plan["tile"] * plan["block_tiles"] + plan["tile"])
    calls, rails_in = call_sizes(row, cfg)
    chans = stream(row, cfg, calls, rails_in)
    main, first = row["passes"]["main"]["name"], row["passes"]["m2" if row["pair"] else "main"]["name"]
    at = 0
    for i, n in enumerate(calls):
        buf = pack_layout([c[at:at + n] for c in chans], cfg["fmt"], layout["block_size"])
        at += n
        got, frames = e.translate(buf)
        want, wframes = o.translate(buf)
        want = want[:wframes * o.frame_bytes]
        assert frames == wframes, (i, frames, wframes)
        if not np.array_equal(got, want):
            bad = np.flatnonzero(got != want)
            raise AssertionError("call %d: %d of %d bytes differ, the first in frame %d of %d" % (i + 1, bad.size, want.size, bad[0] // o.frame_bytes, frames))
        assert [e.peak(c) for c in range(cfg["channels"])] == [o.peak(c) for c in range(cfg["channels"])], i
        assert e.kernel_name() == (first if i == 0 else main), (i, e.kernel_name())
        if i < 2 and exact:
            assert frames >= need if i == 0 else 0 < frames < plan["tile"], (i, frames)
    e.close()
    o.close()
