#!/usr/bin/env python3
"""Every FIR kernel instantiation a probe key can reach, one representative configuration each: tests/golden/kernel_instances.json.

    python tools/kernel_instances.py [tests/golden/kernel_instances.json]          (CPU only: g++ and nothing else)

tools/route_probe.cpp is built the way tests/test_route_cpu.py builds it, its own full sweep (`route_probe keys`) goes through
`route_probe launches -` (the plan of every pass of every key: main; lo, the residual table's pass; m2, the mono pair) and `route_probe
filters -` (does the main pass write the scratch?), and the plans are reduced to COVERAGE UNITS:

  mx, mfma3, px     the kernel's name carries the sample format (KIND, SBY): a unit is (pass, name).  Where the plan writes the scratch
                    (SBY 0, px KIND 4: noise shaping, the cascade, the two passes of 32-bit taps) the second-pass kernels read what it
                    wrote, so there is one unit per bit depth that reaches it: (pass, name, depth).
                    The px kernel alone has two forms of its tile loop under one name, chosen by a runtime argument: a block's channel
                    pair goes through the pipelined epilogue (d2d_px_kernel.h: PIPE, cwn == 2), a single channel (mono, the last of an
                    odd count) through the plain loop.  Its units are split by that form: "pair" (keys of two or more channels) and
                    "single" (keys of an odd count).  The fp6 and int8 kernels only ever convert pairs.
  lut, mfma, mfma2, the epilogue is a runtime argument: a unit is (pass, name, depth, scratch).  Dither and level are dealt round-robin: the
  px_plain          units of a family are taken in sorted order; those whose keys offer several dithers are numbered n = 0, 1, ..., those
                    whose keys all carry one dither (the noise shaper's scratch plans: 'N') are numbered on their own.  Unit n takes
                    dither "TRFXN"[n mod 5], or the next one in that cycle that its keys have, and level (0, -3)[n mod 2], or the other one
                    where its keys lack that: ten consecutive units meet every pair.  Every family must end up with all five dithers and
                    both levels, or the tool fails.

Of the keys that reach a unit (with the unit's dither and level where those were dealt) the representative is the first by: debug flags 0
and kernel AUTO; tap_bits 0; the fewest channels; the sweep's order.

The file holds one row per unit, a row per line: the unit (pass, name, depth or null, scratch, form or null), its family, the key, the decimation M of the
FIR table, the history bytes `keep`, whether the route is `fine` (two passes of 32-bit taps), whether it has a mono pair, and for every pass
the engine has its kernel name, tile (outputs per wave-tile), block_tiles and rows.  tests/test_kernel_instances_cpu.py regenerates the list and
compares it with the file in both directions; tests/test_gpu_kernel_instances.py converts every row's key on the GPU against the oracle.
A new row of a kernel list or a new route condition therefore fails on the CPU until this tool has been run again."""
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "kernel_instances.json")

FAMILIES = ("lut", "mfma", "mfma2", "mfma3", "mx", "px", "px_plain")      # d2d_route.h: FirFamily, in its order
RUNTIME_EPILOGUE = ("lut", "mfma", "mfma2", "px_plain")
PASSES = ("main", "lo", "m2")
DITHERS = "TRFXN"
LEVELS = (0, -3)
KEY = re.compile(r"(\d+):(\d+):(\w):(\d+)([PI])(\d+)([TRFXN]):(-?\d+):(\d+):(\d+):(\d+)$")
KEY_FIELDS = ("dsd_rate", "output_rate", "filter", "channels", "fmt", "bit_depth", "dither", "level_db", "tap_bits", "kernel", "debug")


def parse_key(key):
    """a probe key as the engine's parameters (tools/route_matrix.py: FIELDS)"""
    m = KEY.match(key)
    assert m, key
    return {f: v if f in ("filter", "fmt", "dither") else int(v) for f, v in zip(KEY_FIELDS, m.groups())}


def build_probe(exe):
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    csrc = os.path.join("..", "dsd2dxd_amd", "csrc")
    cmd = ["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"),
           "-o", exe, "route_probe.cpp", os.path.join(csrc, "d2d_route.cpp"), os.path.join(csrc, "d2d_tables.cpp")]
    r = subprocess.run(cmd, cwd=os.path.join(ROOT, "tools"), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return exe


def _probe_many(exe, jobs):
    """[(arguments, standard input)] through the probe side by side: the lines of each job's output"""
    procs = []
    for args, text in jobs:                             # (through files: a pipe would stall every process but the one being read)
        fin, fout = tempfile.TemporaryFile("w+"), tempfile.TemporaryFile("w+")
        fin.write(text)
        fin.seek(0)
        procs.append((subprocess.Popen([exe, *args], stdin=fin, stdout=fout), fin, fout))
    out = []
    for p, fin, fout in procs:
        assert p.wait(timeout=600) == 0, (p.args, p.returncode)
        fout.seek(0)
        out.append(fout.read().rstrip("\n").split("\n"))
        fin.close()
        fout.close()
    return out


def _fields(text):
    head, name = text.split(" name=")                   # (the name holds blanks and comes last)
    return dict([kv.split("=", 1) for kv in head.split(" ")], name=name)


def sweep(exe, workers=None):
    """The probe's full sweep, creatable keys only, in its order: [(key, does the main pass write the scratch?, M, [(pass, family, name,
    the plan's other fields as text)])]."""
    keys = _probe_many(exe, [(["keys"], "")])[0]
    assert len(set(keys)) == len(keys)
    workers = workers or max(1, min(8, (os.cpu_count() or 2) // 2))
    step = -(-len(keys) // workers)
    chunks = ["\n".join(keys[i:i + step]) + "\n" for i in range(0, len(keys), step)]
    outs = _probe_many(exe, [(["launches", "-"], c) for c in chunks] + [(["filters", "-"], c) for c in chunks])
    launches = [l for o in outs[:len(chunks)] for l in o]
    filters = [l for o in outs[len(chunks):] for l in o]
    assert len(launches) == len(filters) == len(keys)
    rows = []
    for key, launch, filt in zip(keys, launches, filters):
        lk, status, *passes = launch.split("\t")
        fk, frest = filt.split("\t", 1)
        assert lk == fk == key
        assert status.startswith("error=") == frest.startswith("error="), (key, launch, filt)
        if status != "ok":
            assert not passes and status.startswith("error="), (key, launch)
            continue
        plans = []
        for p in passes:
            head, name = p.split(" name=")              # (the name holds blanks and comes last)
            ps, family, unit, rest = head.split(" ", 3)
            assert family.startswith("family=") and unit.startswith("unit=") and int(unit[5:]) >= 0, (key, p)
            plans.append((ps, FAMILIES[int(family[7:])], name, rest))
        assert plans[0][0] == "main" and all(p[0] in PASSES for p in plans), (key, launch)
        f = dict(kv.split("=", 1) for kv in frest.split(" "))
        rows.append((key, f["to_scratch"] == "1", int(f["M"]), plans))
    return rows


def _natural(name):
    return (name.split("<")[0], [int(x) for x in re.findall(r"\d+", name)])


def _unit_order(u):
    ps, name, depth, scratch, form = u
    return (PASSES.index(ps), _natural(name), depth or 0, scratch, form or "")


def _preference(cand):
    index, cfg = cand
    return (0 if cfg["debug"] == 0 and cfg["kernel"] == 0 else 1, 0 if cfg["tap_bits"] == 0 else 1, cfg["channels"], index)


def units(exe, rows):
    """The sweep reduced to its coverage units: the golden's rows, in the file's order."""
    cands, family_of, scratch_of = {}, {}, {}
    for index, (key, to_scratch, M, plans) in enumerate(rows):
        cfg = parse_key(key)
        for ps, fam, name, _ in plans:
            # the residual table's pass always writes the scratch; the pair never does (choose_route: no pair under fine, 'N' or a resampler)
            scratch = ps == "lo" or (ps == "main" and to_scratch)
            assert not (ps == "m2" and to_scratch), key
            assert family_of.setdefault(name, fam) == fam
            scratch_of.setdefault((ps, name), set()).add(scratch)
            # the composed polyphase kernel converts a block's channel pair and a single (last odd) channel in two forms of its tile loop
            forms = [None] if fam != "px" else (["pair"] if cfg["channels"] >= 2 else []) + (["single"] if cfg["channels"] % 2 else [])
            for form in forms:
                cands.setdefault((ps, name, cfg["bit_depth"], scratch, form), []).append((index, cfg))
    # families whose name carries the format: the depths of a plan that writes frames are one unit
    merged = {}
    for (ps, name, depth, scratch, form), c in cands.items():
        if family_of[name] not in RUNTIME_EPILOGUE:
            assert len(scratch_of[(ps, name)]) == 1, ("one name, frames and scratch", ps, name)
            if not scratch:
                depth = None
        merged.setdefault((ps, name, depth, scratch, form), []).extend(c)
    chosen = {}
    for fam in FAMILIES:
        mine = sorted((u for u in merged if family_of[u[1]] == fam), key=_unit_order)
        dealt = [0, 0]                                   # units numbered so far: [of one dither, free]
        for u in mine:
            c = merged[u]
            if fam in RUNTIME_EPILOGUE:
                has = sorted({x[1]["dither"] for x in c}, key=DITHERS.index)
                n = dealt[len(has) > 1]
                dealt[len(has) > 1] += 1
                dither = next(d for d in DITHERS[n % 5:] + DITHERS[:n % 5] if d in has)
                c = [x for x in c if x[1]["dither"] == dither]
                level = LEVELS[n % 2] if any(x[1]["level_db"] == LEVELS[n % 2] for x in c) else LEVELS[1 - n % 2]
                c = [x for x in c if x[1]["level_db"] == level]
            chosen[u] = min(c, key=_preference)
        if fam in RUNTIME_EPILOGUE:
            got = [chosen[u][1] for u in mine]
            assert {g["dither"] for g in got} == set(DITHERS) and {g["level_db"] for g in got} == set(LEVELS), (fam, "dithers and levels not all met")
    order = sorted(chosen, key=lambda u: (FAMILIES.index(family_of[u[1]]), _unit_order(u)))
    # the history bytes and `fine` of the representatives: the probe's route lines
    picked = sorted({rows[chosen[u][0]][0] for u in order})
    route = {}
    for line in _probe_many(exe, [(["-"], "\n".join(picked) + "\n")])[0]:
        k, rest = line.split("\t", 1)
        route[k] = _fields(rest)
    out = []
    for u in order:
        key, _, M, plans = rows[chosen[u][0]]
        passes = {}
        for ps, _, name, rest in plans:
            p = dict(kv.split("=", 1) for kv in rest.split(" "))
            passes[ps] = dict(name=name, tile=int(p["tile"]), block_tiles=int(p["block_tiles"]), rows=int(p["rows"]))
        r = route[key]
        assert ("m2" in passes) == (r["mono2_pipe"] != "0") and ("lo" in passes) == (r["fine"] == "1"), (key, r)
        out.append(dict(unit=dict(zip(("pass", "name", "depth", "scratch", "form"), u)), family=family_of[u[1]], key=key, M=M, keep=int(r["keep"]),
                        fine=int(r["fine"]), pair="m2" in passes, passes=passes))
    return out


def unit_id(row):
    """what names a unit in a test id: the pass, the kernel (no blanks), the depth where the unit has one, 's' where it writes the scratch, the
    channel form where the unit has one"""
    u = row["unit"]
    return "%s:%s%s%s%s" % (u["pass"], u["name"].replace(" ", ""), "" if u["depth"] is None else ":%d" % u["depth"],
                            "s" if u["scratch"] and row["family"] in RUNTIME_EPILOGUE else "", ":" + u["form"] if u["form"] else "")


def dumps(rows):
    return "[\n%s\n]\n" % ",\n".join(json.dumps(r, sort_keys=True, separators=(",", ":")) for r in rows)


def generate(exe):
    return units(exe, sweep(exe))


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    with tempfile.TemporaryDirectory() as tmp:
        rows = generate(build_probe(os.path.join(tmp, "route_probe")))
    with open(out, "w") as f:
        f.write(dumps(rows))
    names = {p["name"] for r in rows for p in r["passes"].values()}
    per = {fam: (len({r["unit"]["name"] for r in rows if r["family"] == fam}), sum(r["family"] == fam for r in rows)) for fam in FAMILIES}
    print(len(rows), "units,", len({r["unit"]["name"] for r in rows}), "kernels (", len(names), "names in their engines' plans ) ->", out)
    for fam, (k, n) in per.items():
        print("  %-9s %3d kernels %3d units" % (fam, k, n))


if __name__ == "__main__":
    main()
