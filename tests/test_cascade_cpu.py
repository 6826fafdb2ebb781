"""Filter 'S' (D2D_FILTER_EQUIRIPPLE_CASCADE): the two-stage definition of the 48 kHz multiples, on the CPU.

  * the oracle in cascade mode reproduces tests/golden/cascade_digests.json (tests/golden/make_cascade_golden.py wrote it; the GPU engine is
    held to the same file in tests/test_gpu_cascade.py);
  * choose_filters and choose_route through tools/route_probe.cpp: what 'S' accepts and refuses, that no composed table is chosen and stage A
    writes to the scratch, and the kernel names of every (rate pair, 1 / 2 / 6 / 8 channels, layout, dither T / N, kernel request), pinned in
    tests/golden/route_cascade.json (regenerate: `python tests/test_cascade_cpu.py <route_probe binary>`).  The 'E' rows of the older route
    goldens are tests/test_route_cpu.py's to hold;
  * what the change of definition costs, oracle against oracle, printed per rate pair (pytest -s shows the table; DESIGN.md section 0 quotes it).
"""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

from cascade_cases import COMPOSED, CONTROL, call_buffers, golden_cases, make_channels, oracle_run, pair_id  # noqa: E402
from helpers import decode_pcm, pack_layout, synth  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
D2D_ERR_PARAM, D2D_ERR_FILTER = -1, -3


def _digests():
    with open(os.path.join(GOLDEN, "cascade_digests.json")) as f:
        return json.load(f)


# ---- the pins ------------------------------------------------------------------------------------------------------------------------

def test_the_digest_file_holds_the_cases():
    d = _digests()
    cases = golden_cases()
    assert sorted(d) == sorted(cases)
    for name, (kw, calls, recipe) in cases.items():
        assert d[name]["kw"] == kw and d[name]["calls"] == list(calls) and d[name]["input"] == recipe, name
    pairs = {(v["kw"]["dsd_rate"], v["kw"]["output_rate"]) for v in d.values() if v["kw"]["bit_depth"] == 24 and v["kw"]["dither"] == "T"}
    assert pairs == set(COMPOSED + CONTROL)
    assert {(v["kw"]["bit_depth"], v["kw"]["dither"]) for v in d.values()} >= {(24, "T"), (32, "F"), (24, "N"), (16, "T")}
    assert any(v["kw"]["channels"] == 6 and v["kw"]["bit_depth"] == 16 for v in d.values())
    assert os.path.getsize(os.path.join(GOLDEN, "cascade_digests.json")) < 100_000


@pytest.mark.parametrize("name", sorted(golden_cases()))
def test_oracle_cascade_mode_reproduces_the_digest(oracle_mod, name):
    g = _digests()[name]
    kw = g["kw"]
    bufs = call_buffers(make_channels(g["input"]), g["calls"], kw["fmt"], kw["block_size"])
    pcm, frames, peaks = oracle_run(oracle_mod, kw, bufs)
    fb = kw["channels"] * (2 if kw["bit_depth"] == 16 else 4 if kw["bit_depth"] == 32 else 3)
    assert frames == g["frames"] and pcm.size == sum(frames) * fb
    assert pcm[:32 * fb].tobytes().hex() == g["head"]
    assert hashlib.sha256(pcm.tobytes()).hexdigest() == g["sha256"]
    assert peaks == g["peaks"] and all(p > 0.0 for p in peaks)


# ---- choose_filters / choose_route -----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("route_probe_s") / "route_probe")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    csrc = os.path.join("..", "dsd2dxd_amd", "csrc")
    cmd = ["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"),
           "-o", exe, "route_probe.cpp", os.path.join(csrc, "d2d_route.cpp"), os.path.join(csrc, "d2d_tables.cpp")]
    r = subprocess.run(cmd, cwd=os.path.join(ROOT, "tools"), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return exe


def _ask(exe, keys, *mode):
    p = subprocess.run([exe, *mode, "-"], input="\n".join(keys) + "\n", capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, (p.stdout[-500:], p.stderr[-500:])
    lines = [l.split("\t", 1) for l in p.stdout.strip().split("\n")]
    assert [k for k, _ in lines] == list(keys)
    return dict(lines)


def _key(dr, rate, filt, ch=2, fmt="P", bits=24, dither="T", level=0, tap_bits=0, kernel=0, dbg=0):
    return "%d:%d:%s:%d%s%d%s:%d:%d:%d:%d" % (dr, rate, filt, ch, fmt, bits, dither, level, tap_bits, kernel, dbg)


def route_keys(filt="S"):
    """every (pair, channels, layout, dither, kernel request) the route golden pins"""
    return [_key(dr, rate, filt, ch=ch, fmt=fmt, dither=di, kernel=k) for dr, rate in COMPOSED + CONTROL for ch in (1, 2, 6, 8) for fmt in "PI" for di in "TN"
            for k in (0, 1, 2)]


def test_s_is_refused_outside_the_48k_family(probe):
    keys = [_key(dr, rate, "S") for dr, rate in ((1, 88200), (1, 176400), (1, 352800), (2, 88200), (2, 705600), (4, 1411200), (8, 352800))]
    for k, rest in _ask(probe, keys).items():
        assert rest.startswith("error=%d:" % D2D_ERR_FILTER) and "two-stage" in rest and "48 kHz multiples only" in rest, (k, rest)
    # a rate pair nobody serves is a rate error under every letter, 'S' included
    got = _ask(probe, [_key(8, 88200, "S"), _key(8, 88200, "E"), _key(1, 48000, "S")])
    assert got[_key(8, 88200, "S")] == got[_key(8, 88200, "E")] == "error=-2:DSD512 input: only 352800 output is available"
    assert got[_key(1, 48000, "S")] == "error=-2:Invalid output rate"


def test_the_older_messages_stand_word_for_word(probe):
    got = _ask(probe, [_key(1, 96000, f) for f in "XDC"] + [_key(1, 96000, "Q"), _key(1, 96000, "S", tap_bits=32), _key(1, 96000, "E", tap_bits=32)])
    for f in "XDC":
        assert got[_key(1, 96000, f)] == "error=-3:48 kHz multiples are only available with the equiripple filter"
    assert got[_key(1, 96000, "Q")] == "error=-3:Invalid filter type; must be E, X, D or C"
    # 32-bit taps: refused for 'S' as for every resampled rate
    want = "error=%d:32-bit taps serve the 44.1k-family rates with dither T, R, F or X" % D2D_ERR_PARAM
    assert got[_key(1, 96000, "S", tap_bits=32)] == got[_key(1, 96000, "E", tap_bits=32)] == want


def test_s_chooses_stage_a_into_the_scratch_and_no_composed_table(probe):
    keys = route_keys()
    got = _ask(probe, keys, "filters")
    for k in keys:
        dr, rate = (int(v) for v in k.split(":")[:2])
        f = dict(kv.split("=") for kv in got[k].split(" ")) if not got[k].startswith("error") else None
        if f is None:                                   # (only an explicit D2D_KERNEL_MFMA request can be refused: the route's LDS check)
            assert k.split(":")[-2] == "2" and got[k].startswith("error=-1:MFMA kernel does not support"), (k, got[k])
            continue
        assert f == dict(fir="A_M%d" % (8 * dr), M=str(8 * dr), resamp="%d/147/%s" % (rate // 2400, f["resamp"].split("/")[2]), poly="-", cascade="1",
                         to_scratch="1"), (k, got[k])
    # the same keys under 'E': a composed table on the eight pairs, the cascade on the two others
    for k, rest in _ask(probe, route_keys("E"), "filters").items():
        if rest.startswith("error"):
            continue
        dr, rate = (int(v) for v in k.split(":")[:2])
        f = dict(kv.split("=") for kv in rest.split(" "))
        assert (f["poly"] == "-") == ((dr, rate) in CONTROL) and (f["cascade"] == "1") == ((dr, rate) in CONTROL), (k, rest)


def _names(exe):
    """key -> [what d2d_kernel_name predicts, the main pass's launch plan], or the create error"""
    keys = route_keys()
    routes, launches = _ask(exe, keys), _ask(exe, keys, "launches")
    out = {}
    for k in keys:
        if routes[k].startswith("error"):
            assert launches[k] == routes[k]
            out[k] = routes[k]
            continue
        status, main = launches[k].split("\t")[:2]
        assert status == "ok" and main.startswith("main ") and " unit=-1 " not in main, (k, launches[k])       # (a compiled kernel serves every plan)
        out[k] = [routes[k].split(" name=")[1], main.split(" name=")[1]]
    return out


def _grouped(names):
    groups = {}
    for k, v in names.items():
        groups.setdefault(json.dumps(v), []).append(k)
    return [[json.loads(v), ks] for v, ks in sorted(groups.items())]


def test_s_kernel_names_equal_the_golden(probe):
    with open(os.path.join(GOLDEN, "route_cascade.json")) as f:
        golden = {k: v for v, ks in json.load(f) for k in ks}
    got = _names(probe)
    assert sorted(got) == sorted(golden)
    bad = [(k, got[k], golden[k]) for k in got if got[k] != golden[k]]
    assert not bad, (len(bad), bad[:3])
    # stage A of an 'S' engine is never a frame kernel or the composed one
    for k, v in got.items():
        if isinstance(v, list):
            assert "px" not in v[0] and "poly" not in v[0], (k, v)


def test_s_takes_the_routes_e_takes_where_e_is_two_stage(probe):
    """DSD256 -> 96 kHz and DSD512: the whole route line and every launch plan, letter apart"""
    ks = [k for k in route_keys() if tuple(int(v) for v in k.split(":")[:2]) in CONTROL]
    ke = [k.replace(":S:", ":E:") for k in ks]
    for mode in ((), ("launches",)):
        s, e = _ask(probe, ks, *mode), _ask(probe, ke, *mode)
        assert [s[a] for a in ks] == [e[b] for b in ke]
    # ... and on the eight other pairs an 'S' engine runs the kernels of the same shape that DSD256 -> 96 kHz runs: the scratch
    # flavour (last two template arguments 0) of a pipelined kernel for stereo under AUTO
    got = _names(probe)
    for dr, rate in COMPOSED:
        for fmt in "PI":
            name = got[_key(dr, rate, "S", fmt=fmt)][1]
            assert name.startswith(("d2d_fir_mfma3_kernel<", "d2d_fir_mx_kernel<")), name
            args = name[name.index("<") + 1:-1].split(", ")
            assert args[0] == str(dr) and args[3:5] == ["0", "0"], name


# ---- what the definition costs ---------------------------------------------------------------------------------------------------------

def test_difference_table_between_the_two_definitions(oracle_mod):
    """0.25 s of stereo DSD (left a 1 kHz sine at -9 dBFS, right pink noise), converted by the oracle under both definitions: the fraction of
    24-bit TPDF samples that move and by how many LSB at most, and the RMS difference of the float output (FS = 1).  Asserted: something moves on
    each of the eight composed pairs, nothing at all on the two pairs that are the cascade under both letters."""
    rows = []
    for dr, rate in COMPOSED + CONTROL:
        n = 2822400 * dr // 8 // 4
        chans = [synth("sine", n, seed=11, dsd_rate=dr), synth("pink", n, seed=12, amp=0.098, dsd_rate=dr)]
        buf = [pack_layout(chans, "P", 4096)]
        base = dict(dsd_rate=dr, output_rate=rate, channels=2, fmt="P", endianness="L", block_size=4096, seed=5)
        i_s, fr_s, _ = oracle_run(oracle_mod, dict(base, bit_depth=24, dither="T"), buf, cascade=True)
        i_e, fr_e, _ = oracle_run(oracle_mod, dict(base, bit_depth=24, dither="T"), buf, cascade=False)
        f_s, _, _ = oracle_run(oracle_mod, dict(base, bit_depth=32, dither="X"), buf, cascade=True)
        f_e, _, _ = oracle_run(oracle_mod, dict(base, bit_depth=32, dither="X"), buf, cascade=False)
        assert fr_s == fr_e and fr_s[0] > 0                       # the same frame counts under both definitions
        d = np.abs(decode_pcm(i_s, 24, 2) - decode_pcm(i_e, 24, 2))
        df = decode_pcm(f_s, 32, 2).astype(np.float64) - decode_pcm(f_e, 32, 2).astype(np.float64)
        rows.append((dr, rate, float((d != 0).mean()), int(d.max()), float(np.sqrt((df ** 2).mean())), np.array_equal(i_s, i_e) and np.array_equal(f_s, f_e)))
    print("\n| rate pair | 24-bit TPDF samples that move | worst, LSB | float output, RMS difference |\n|---|---|---|---|")
    for dr, rate, moved, worst, rms, same in rows:
        print("| DSD%d -> %g kHz | %.1f %% | %d | %.1e |" % (64 * dr, rate / 1000, 100 * moved, worst, rms))
    for dr, rate, moved, worst, rms, same in rows:
        if (dr, rate) in CONTROL:
            assert same and moved == 0.0 and worst == 0 and rms == 0.0, pair_id(dr, rate)
        else:
            assert not same and moved > 0.0 and worst > 0 and rms > 0.0, pair_id(dr, rate)


if __name__ == "__main__":
    # regenerate tests/golden/route_cascade.json from a route_probe binary
    with open(os.path.join(GOLDEN, "route_cascade.json"), "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(g, separators=(",", ":")) for g in _grouped(_names(sys.argv[1]))) + "\n]\n")
