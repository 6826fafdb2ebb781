#!/usr/bin/env python3
"""The kernel route of every configuration of tools/engine_matrix.py, as an MI355X reported it: tests/golden/route_matrix.json.

    python tools/route_matrix.py MATRIX.jsonl tests/golden/route_matrix.json

Each row of the sweep is reduced to its outcome -- the create error, or kernel_name() before the call, kernel_name() after it, info() and the
kernel, table_variant and fir_bytes of the exported blob's header (null where the export is refused) -- and the configurations are grouped by
identical outcome, every configuration of the sweep in exactly one group.  load() gives [{"outcome": {...}, "configurations": [term, ...]},
...]; the file holds the same as rows, a group per line: "names" the distinct kernel names, "infos" the distinct info() dictionaries,
"groups" rows of COLUMNS (the names and info as indices into those lists; the three header fields null where there is no header), "errors"
rows of [code, text, terms].  A term is a product of value lists, one per field of FIELDS, "1:88200:E:1,2:P,I:16,24:T:0:0:0,1:0": expand() gives its keys.  A
key is tools/route_probe.cpp's: <dsd_rate>:<output_rate>:<filter>:<channels><fmt><depth><dither>:<level>:<tap_bits>:<kernel>:<debug flags>.
tests/test_route_cpu.py holds d2d_route.cpp to the file on the CPU, tests/test_gpu_route.py one engine per group on the GPU."""
import itertools
import json
import sys

COLUMNS = ("kernel_name", "kernel_name_after", "info", "kernel", "table_variant", "fir_bytes", "configurations")
FIELDS = ("dsd_rate", "output_rate", "filter", "channels", "fmt", "bit_depth", "dither", "level_db", "tap_bits", "kernel", "debug")


def key(cfg):
    return "%d:%d:%s:%d%s%d%s:%d:%d:%d:%d" % tuple(cfg[f] for f in FIELDS)


def expand(term):
    """the keys of a term"""
    return ["%s:%s:%s:%s%s%s%s:%s:%s:%s:%s" % c for c in itertools.product(*(v.split(",") for v in term.split(":")))]


def terms(cfgs):
    """configurations as few products as merging along one field at a time finds, last field first or first field first"""
    best = None
    for order in (range(len(FIELDS) - 1, -1, -1), range(len(FIELDS))):
        ts = [tuple((str(int(c[f]) if f == "level_db" else c[f]),) for f in FIELDS) for c in cfgs]
        n = 0
        while n != len(ts):
            n = len(ts)
            for f in order:
                rest = {}
                for t in ts:
                    rest.setdefault(t[:f] + t[f + 1:], []).extend(t[f])
                ts = [r[:f] + (tuple(v),) + r[f:] for r, v in rest.items()]
        if best is None or len(ts) < len(best):
            best = ts
    return [":".join(",".join(v) for v in t) for t in best]


def outcome(row):
    """the part of an engine_matrix.py row that the route decides"""
    if "create_error" in row:
        return dict(create_error=row["create_error"])
    return dict(kernel_name=row["kernel_name"], kernel_name_after=row["kernel_name_after"], info=row["info"], header=row.get("header"))


def load(path):
    with open(path) as f:
        d = json.load(f)
    assert tuple(d["columns"]) == COLUMNS
    out = [dict(outcome=dict(create_error=[code, text]), configurations=ts) for code, text, ts in d["errors"]]
    for name, after, info, kernel, variant, fir_bytes, ts in d["groups"]:
        header = None if kernel is None else dict(kernel=kernel, table_variant=variant, fir_bytes=fir_bytes)
        out.append(dict(outcome=dict(kernel_name=d["names"][name], kernel_name_after=d["names"][after], info=d["infos"][info], header=header),
                        configurations=ts))
    return out


def main():
    groups = {}
    n = 0
    with open(sys.argv[1]) as f:
        for line in f:
            row = json.loads(line)
            groups.setdefault(json.dumps(outcome(row), sort_keys=True), []).append(row)
            n += 1
    names, infos, rows, errors = [], [], [], []
    for o, c in sorted(groups.items()):
        o = json.loads(o)
        if "create_error" in o:
            errors.append(o["create_error"] + [terms(c)])
            continue
        for v, seen in ((o["kernel_name"], names), (o["kernel_name_after"], names), (o["info"], infos)):
            if v not in seen:
                seen.append(v)
        h = o["header"] or dict(kernel=None, table_variant=None, fir_bytes=None)
        rows.append([names.index(o["kernel_name"]), names.index(o["kernel_name_after"]), infos.index(o["info"]), h["kernel"], h["table_variant"], h["fir_bytes"], terms(c)])
    dumps = lambda v: json.dumps(v, sort_keys=True, separators=(",", ":"))
    lines = lambda name, v: '"%s":[\n%s\n]' % (name, ",\n".join(dumps(x) for x in v))
    with open(sys.argv[2], "w") as f:
        f.write('{"columns":%s,\n%s,\n%s,\n%s,\n%s}\n' % (dumps(COLUMNS), lines("names", names), lines("infos", infos), lines("errors", errors),
                                                       lines("groups", rows)))
    print(n, "configurations in", len(groups), "groups ->", sys.argv[2])


if __name__ == "__main__":
    main()
