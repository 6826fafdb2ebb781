#!/usr/bin/env python3
"""Regenerate tests/golden/cascade_digests.json: the two-stage definition of the 48 kHz multiples (filter 'S') as the CPU oracle computes it in
its cascade mode (Oracle.use_cascade()).

PARITY UNPINNED, like make_golden.py: the vectors pin this repository's oracle and, through it, the GPU engine's 'S' route; nothing here comes
from the reference.  Per entry: the engine parameters, the input recipe (seeded helpers.synth / helpers.random_bytes per channel) and the call
sizes in bytes per channel, the frames of every call, the SHA-256 of all PCM, the first 32 frames in hex and the per-channel peaks.  The cases
are tests/cascade_cases.py: golden_cases().

  python tests/golden/make_cascade_golden.py        (run from the repo root)
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from cascade_cases import digest_entry, golden_cases  # noqa: E402
from oracle import oracle as O  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))


def main():
    O.build()
    out = {name: digest_entry(O, kw, calls, recipe) for name, (kw, calls, recipe) in golden_cases().items()}
    path = os.path.join(HERE, "cascade_digests.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", len(out), "entries,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
