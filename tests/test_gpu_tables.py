"""An engine uploads what the builders of dsd2dxd_amd/csrc/d2d_tables.cpp built: the exported table blob of every kernel route against
tests/golden/table_digests.json, the digests tools/table_probe.cpp prints on the CPU (tests/test_tables_cpu.py).

One engine per route of tests/test_gpu_long_streams.py (n_files = 1), no conversion.  The blob's header (TableBlobHeader, d2d_internal.h)
names filter type, taps, M, bit order and table variant; those fields pick the golden line, so the test predicts no route.  The FIR part and
the stage-B part are hashed as the probe hashes them.  Engines on two-pass 32-bit taps hold two tables and export none: left out.  Variant 7
(the plain polyphase kernel) is D2D_POLYS[..].q itself, taken here from filters/filter_tables.json."""
import json
import os
import struct

import numpy as np
import pytest

from test_gpu_long_streams import NS_ROUTES, ROUTES

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = struct.Struct("<10I2Q")      # magic, abi, kernel, endianness, ntaps, M, scale_bits, filter_type, table_variant, reserved, fir_bytes, resamp_bytes
KIND_OF_VARIANT = {2: "two_group", 3: "pipelined", 5: "fp6", 8: "fp6_wide"}
VARIANTS = {0, 2, 3, 5, 6, 7, 8}
seen = set()


def _cases():
    out = {}
    for name, (kw, kernel) in {**ROUTES, **NS_ROUTES}.items():
        if kw.get("tap_bits") == 32 and not kernel.endswith(", 7>"):      # two passes: not the seven-digit kernel
            continue
        out[name] = kw
    # the other bit order
    out["fp6_m32_t24_msb"] = dict(ROUTES["fp6_m32_t24"][0], endianness="M")
    out["lut_176k_msb"] = dict(ROUTES["lut_176k"][0], endianness="M")
    return out


CASES = _cases()


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "table_digests.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def polys():
    with open(os.path.join(ROOT, "filters", "filter_tables.json")) as f:
        return json.load(f)["polys"]


def _line(b):
    """"<bytes> <64-bit FNV-1a>" as tools/table_probe.cpp prints it"""
    h = 0xcbf29ce484222325
    for x in bytes(b):
        h = ((h ^ x) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
    return "%d %016x" % (len(b), h)


@pytest.mark.parametrize("name", list(CASES))
def test_engine_uploads_the_tables_the_builders_built(engine_lib, golden, polys, name):
    import torch
    kw = CASES[name]
    e = engine_lib.Engine(n_files=1, filter="E", **kw)
    nb = e.tables_bytes()
    blob = torch.zeros(nb, dtype=torch.uint8, device="cuda")
    e.tables_export_device(blob.data_ptr(), nb)
    torch.cuda.synchronize()
    b = blob.cpu().numpy().tobytes()
    magic, abi, kernel, endianness, ntaps, M, S, ftype, variant, _, fir_bytes, resamp_bytes = HEADER.unpack_from(b)
    assert magic == 0x54443244 and HEADER.size + ((fir_bytes + 15) & ~15) + resamp_bytes == nb
    assert endianness == (1 if kw["endianness"] == "M" else 0)
    fir = b[HEADER.size:HEADER.size + fir_bytes]
    if variant in (6, 7):
        assert ftype == ord("P")
        p, = [p for p in polys if (p["Mp"], p["NP"]) == (M, ntaps)]
        assert S == p["S"] and resamp_bytes == 0
        if variant == 7:
            assert fir == np.array(p["q"], dtype="<i4").tobytes()
        else:
            assert _line(fir) == golden[p["name"] + "/px"]
    else:
        kind = KIND_OF_VARIANT[variant] if variant else ("lut" if kernel == engine_lib.KERNEL_LUT else "one_group")
        key = "%c_M%d/%s/%s" % (ftype, M, "LM"[endianness], kind)
        assert _line(fir) == golden[key], key
        assert (resamp_bytes != 0) == (ftype == ord("A"))
        if resamp_bytes:
            off = HEADER.size + ((fir_bytes + 15) & ~15)
            assert _line(b[off:off + resamp_bytes]) == golden["B_%d/resamp2" % kw["output_rate"]]
    seen.add(variant)


def test_every_table_variant_was_seen():
    """(runs after the cases above: the route lists reach every variant by themselves)"""
    assert seen == VARIANTS
