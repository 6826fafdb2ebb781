#!/usr/bin/env python3
"""What one rank of an N-way split of BASELINE config 5 costs (DSD512, 8 channels byte-interleaved MSB-first -> 96 kHz 24-bit TPDF),
for the two ways the stream can be cut -- run on the GPU box from the repository root, outside pytest:

  (a) whole   one step over the whole batch
  (b) time    every file sought to slice r of N (dsd2dxd_amd.shard.shard_time), primed with the halo and converted: prime + translate timed together
  (c) channel the one-channel share of a channel split (channel_first = r, channel_count = 1): reads the whole interleaved stream

One process, seeded random bytes distinct per file, the cases alternated after a warm-up round; per case the device time
(d2d_profile_read_all: every kernel of the calls) and a host clock that ends in a synchronise.  Prints one JSON line; no threshold:
the numbers go to profiles/timeslice_check.md."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import dsd2dxd_amd as d  # noqa: E402
from dsd2dxd_amd.shard import shard_time  # noqa: E402

CH = 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=16)
    ap.add_argument("--seconds", type=float, default=60.0, help="audio seconds per file")
    ap.add_argument("--world", type=int, default=8)
    ap.add_argument("--rank", type=int, default=3, help="the slice / the channel that is timed")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--seed", type=int, default=206)
    args = ap.parse_args()
    assert args.reps >= 5 and 0 <= args.rank < args.world <= CH
    dev = torch.device("cuda", 0)
    kw = dict(dsd_rate=8, output_rate=96000, channels=CH, fmt="I", endianness="M", block_size=1, filter="E", bit_depth=24, dither="T", seed=args.seed)
    bpc = max(1, int(round(args.seconds * 2822400 * 8 / 8 / 4096))) * 4096
    gen = torch.Generator(device=dev)
    gen.manual_seed(args.seed)
    files = [torch.randint(0, 256, (bpc * CH,), dtype=torch.uint8, device=dev, generator=gen) for _ in range(args.files)]
    whole = d.Engine(n_files=args.files, **kw)
    part = d.Engine(n_files=args.files, **kw)
    chan = d.Engine(n_files=args.files, channel_first=args.rank, channel_count=1, **kw)
    # interleaved input: byte p of every channel sits at p * CH; the batch entry points want 16-byte aligned pointers, so cut at even positions
    halo, begin, end = shard_time(bpc, args.world, args.rank, align=2, preroll=part.preroll_bytes())

    def ios_for(eng, a, z, outs):
        ios = (d.FileIO * args.files)()
        for i, f in enumerate(files):
            ios[i].dsd = f.data_ptr() + a * CH; ios[i].bytes_per_channel = z - a
            if outs is not None:
                ios[i].pcm = outs[i].data_ptr(); ios[i].pcm_capacity_bytes = outs[i].numel()
        return ios

    def outs_for(eng, frames):
        return [torch.empty((frames * eng.frame_bytes + 31) // 16 * 16, dtype=torch.uint8, device=dev) for _ in range(args.files)]

    out_whole = outs_for(whole, whole.next_frames(bpc))
    part.seek(begin)
    out_part = outs_for(part, part.next_frames(end - begin))
    out_chan = outs_for(chan, chan.next_frames(bpc))
    io_whole, io_chan = ios_for(whole, 0, bpc, out_whole), ios_for(chan, 0, bpc, out_chan)
    io_halo, io_part = ios_for(part, halo, begin, None), ios_for(part, begin, end, out_part)

    def timed(eng, calls):
        eng.profile_enable(True)
        eng.profile_read_all()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for c in calls:
            c()
        torch.cuda.synchronize()
        host = (time.perf_counter() - t0) * 1e3
        _, step, _ = eng.profile_read_all()
        return step, host

    def case_whole():
        whole.reset()
        return timed(whole, [lambda: whole.translate_batch_device(io_whole)])

    def case_time():
        for f in range(args.files):
            part.seek(halo, file=f)
        return timed(part, [lambda: part.prime_batch_device(io_halo), lambda: part.translate_batch_device(io_part)])

    def case_chan():
        chan.reset()
        return timed(chan, [lambda: chan.translate_batch_device(io_chan)])

    cases = {"whole": case_whole, "time": case_time, "channel": case_chan}
    for fn in cases.values():                                   # warm-up: buffers grown, kernels loaded
        fn()
    rec = {k: [] for k in cases}
    for _ in range(args.reps):
        for k, fn in cases.items():
            rec[k].append(fn())
    out = {"files": args.files, "seconds_per_file": round(bpc * 8 / (2822400 * 8), 3), "bytes_per_channel": bpc, "world": args.world, "rank": args.rank,
           "slice": [halo, begin, end], "preroll_bytes": part.preroll_bytes(), "reps": args.reps,
           "kernels": {"whole": whole.kernel_name(), "time": part.kernel_name(), "channel": chan.kernel_name()}}
    for k, v in rec.items():
        devs, hosts = [x[0] for x in v], [x[1] for x in v]
        out[k] = {"device_ms_median": round(statistics.median(devs), 3), "device_ms_min": round(min(devs), 3), "device_ms_max": round(max(devs), 3),
                  "host_ms_median": round(statistics.median(hosts), 3), "host_ms_min": round(min(hosts), 3), "host_ms_max": round(max(hosts), 3)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
