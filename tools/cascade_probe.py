#!/usr/bin/env python3
"""The two definitions of the 48 kHz multiples side by side on the bench batch shape (GPU box, repo root):

    python tools/cascade_probe.py [OUT.md] [--files 64] [--seconds 60]

For each of the eight rate pairs that filter 'E' serves with a composed one-pass table, and for each of 'E' and 'S' (the two-stage cascade:
stage A into the scratch, stage B out of it), one device-resident batch of --files stereo files of --seconds each, planar 4096-byte blocks,
24-bit TPDF: a warm-up call, then five timed calls on a reset engine.  Reported: the median FIR time and the median whole-step time of
d2d_profile_read_all (device events around the FIR launch and around every kernel of the call), the spread of the step times, and the
kernel d2d_kernel_name names after the call.  Under 'S' the FIR time is stage A alone and the rest of the step is stage B; under 'E' the
composed kernel is the whole step.  Every file has its own random input.  The table goes to stdout and, when a path is given, to that file."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import dsd2dxd_amd as d  # noqa: E402

PAIRS = [(1, 96000), (1, 192000), (1, 384000), (2, 96000), (2, 192000), (2, 384000), (4, 192000), (4, 384000)]
RUNS = 5


def measure(dsd_rate, out_rate, filt, files, seconds):
    kw = dict(dsd_rate=dsd_rate, output_rate=out_rate, channels=2, fmt="P", endianness="L", block_size=4096, filter=filt, bit_depth=24, dither="T", seed=1)
    e = d.Engine(n_files=files, **kw)
    n = int(seconds * 2822400 * dsd_rate / 8 / 4096) * 4096
    buf = torch.randint(0, 256, (files, n * 2), dtype=torch.uint8, device="cuda")
    frames = e.next_frames(n)
    out = torch.zeros((files, (frames * e.frame_bytes + 31) // 16 * 16), dtype=torch.uint8, device="cuda")
    ios = (d.FileIO * files)()
    for i in range(files):
        ios[i].dsd = buf[i].data_ptr(); ios[i].bytes_per_channel = n
        ios[i].pcm = out[i].data_ptr(); ios[i].pcm_capacity_bytes = frames * e.frame_bytes
    firs, steps = [], []
    for it in range(RUNS + 1):                        # the first call warms up: code objects, the scratch grows to the call's size
        e.reset()
        e.profile_enable(True)
        e.translate_batch_device(ios)
        torch.cuda.synchronize()
        fir, step, _ = e.profile_read_all()
        if it:
            firs.append(fir)
            steps.append(step)
    name = e.kernel_name()
    e.close()
    del buf, out
    torch.cuda.empty_cache()
    return statistics.median(firs), statistics.median(steps), min(steps), max(steps), name, frames * 2 * files


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?", default="")
    ap.add_argument("--files", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=60.0)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "cascade_probe.py measures on the GPU"
    lines = ["%d files x %g s, stereo, planar 4096-byte blocks, 24-bit TPDF; median of %d calls after a warm-up call; %s" %
             (args.files, args.seconds, RUNS, torch.cuda.get_device_name(0)), "",
             "| rate pair | filter | FIR ms | step ms | step min .. max | Gsamples/s (step) | kernel |", "|---|---|---|---|---|---|---|"]
    for dsd_rate, out_rate in PAIRS:
        for filt in "ES":
            fir, step, lo, hi, name, outs = measure(dsd_rate, out_rate, filt, args.files, args.seconds)
            lines.append("| DSD%d -> %g kHz | %s | %.2f | %.2f | %.2f .. %.2f | %.1f | `%s` |" %
                         (64 * dsd_rate, out_rate / 1000, filt, fir, step, lo, hi, outs / step / 1e6, name))
            print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
