#!/usr/bin/env python3
"""What the host engine decides and computes, one JSON line per configuration: the counterpart of isa_digest.py for d2d_engine.cpp.

    python tools/engine_matrix.py OUT.jsonl [--every N]      (the library: D2D_AMD_LIB, else the tree's)

For every configuration of the sweep an engine is created and the line holds either the create error (code and text) or kernel_name() before
any call, info(), frame_bytes, tables_bytes(), preroll_bytes(), slice_align_bytes(), the sha256 of the exported table blob and the kernel,
table_variant and fir_bytes of its header (or the refusal), and after one translate of two 4096-byte blocks per channel of seeded random
input the sha256 of the output, the frame count, the peaks and kernel_name() again.  A change of host code that must leave every create-time
decision, table, job table and launch argument alone gives the same file with the library before and after it (`cmp`).  --every N keeps
one configuration in N (a quick look)."""
import argparse
import hashlib
import itertools
import json
import os
import struct
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

import dsd2dxd_amd as d  # noqa: E402
from test_gpu_parity import RATE_MATRIX  # noqa: E402

FLAGS = [("NO_COOP", d.DBG_NO_COOP), ("NO_MX", d.DBG_NO_MX), ("NO_PIPE", d.DBG_NO_PIPE), ("MFMA_V1", d.DBG_MFMA_V1),
         ("TAPS32_2PASS", d.DBG_TAPS32_2PASS)]


def configurations():
    for (dsd_rate, out_rate, filt), ch, fmt, bits, dither, level, tap_bits, kernel in itertools.product(
            RATE_MATRIX, (1, 2, 3, 8), "PI", (16, 24, 32), "TFN", (0.0, -3.0), (0, 32), (0, 1)):
        yield dict(dsd_rate=dsd_rate, output_rate=out_rate, filter=filt, channels=ch, fmt=fmt, bit_depth=bits, dither=dither, level_db=level,
                   tap_bits=tap_bits, kernel=kernel, debug=0)
    # the diagnostic routes, on stereo: each flag alone, the matrix-core kernel asked for by name too
    for (dsd_rate, out_rate, filt), fmt, bits, dither, tap_bits, kernel, (_, flag) in itertools.product(
            RATE_MATRIX, "PI", (24, 32), "TN", (0, 32), (0, 2), FLAGS):
        yield dict(dsd_rate=dsd_rate, output_rate=out_rate, filter=filt, channels=2, fmt=fmt, bit_depth=bits, dither=dither, level_db=0.0,
                   tap_bits=tap_bits, kernel=kernel, debug=flag)


def describe(cfg, data):
    kw = dict(cfg, endianness="L" if cfg["fmt"] == "P" else "M", block_size=4096, seed=7)
    row = dict(cfg)
    try:
        e = d.Engine(**kw)
    except d.D2DError as ex:
        row["create_error"] = [ex.code, ex.message]
        return row
    row.update(kernel_name=e.kernel_name(), info=e.info(), frame_bytes=e.frame_bytes, tables_bytes=e.tables_bytes(),
               preroll_bytes=e.preroll_bytes(), slice_align_bytes=e.slice_align_bytes())
    nb = e.tables_bytes()
    blob = torch.zeros(nb, dtype=torch.uint8, device="cuda")
    try:
        e.tables_export_device(blob.data_ptr(), nb)
        torch.cuda.synchronize()
        raw = blob.cpu().numpy().tobytes()
        row["tables"] = hashlib.sha256(raw).hexdigest()
        kernel, variant, fir_bytes = struct.unpack_from("<8xI20xI4xQ", raw)          # TableBlobHeader (d2d_internal.h)
        row["header"] = dict(kernel=kernel, table_variant=variant, fir_bytes=fir_bytes)
    except d.D2DError as ex:
        row["tables"] = [ex.code, ex.message]
    pcm, frames = e.translate(data[:2 * 4096 * cfg["channels"]])
    row.update(pcm=hashlib.sha256(pcm.tobytes()).hexdigest(), frames=frames, peaks=[e.peak(c) for c in range(cfg["channels"])],
               kernel_name_after=e.kernel_name())
    e.close()
    return row


def call_buffer():
    return np.random.default_rng(206).integers(0, 256, 2 * 4096 * 8, dtype=np.uint8)     # (any byte string is a call buffer in either layout)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--every", type=int, default=1)
    args = ap.parse_args()
    data = call_buffer()
    n = 0
    with open(args.out, "w") as f:
        for i, cfg in enumerate(configurations()):
            if i % args.every:
                continue
            f.write(json.dumps(describe(cfg, data), sort_keys=True) + "\n")
            n += 1
            if n % 1000 == 0:
                print(n, "configurations", flush=True)
    print(n, "configurations ->", args.out, "library", d.library_path())


if __name__ == "__main__":
    main()
