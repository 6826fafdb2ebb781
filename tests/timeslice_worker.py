"""One rank of the time-partition test (tests/test_gpu_timeslice_ranks.py): takes its slice of ONE 8-channel stream
(dsd2dxd_amd.shard.shard_time), seeks, primes with the halo and converts the slice in two device-resident calls.
usage: timeslice_worker.py <rank> <world> <out.npz>"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

NBYTES, CHN = 24776, 8
# BASELINE config 5's shape: DSD512, 8 channels byte-interleaved MSB-first -> 96 kHz 24-bit TPDF
KW = dict(dsd_rate=8, output_rate=96000, channels=CHN, fmt="I", endianness="M", block_size=1, filter="E", bit_depth=24, dither="T", seed=512)


def stream_channels():
    from helpers import random_bytes
    return [random_bytes(NBYTES, 700 + c) for c in range(CHN)]


def main():
    rank, world, out = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3]
    import torch
    import dsd2dxd_amd as d
    from dsd2dxd_amd.shard import shard_time
    from helpers import pack_layout
    dev = torch.device("cuda", 0)
    eng = d.Engine(device=0, **KW)
    halo, begin, end = shard_time(NBYTES, world, rank, preroll=eng.preroll_bytes())
    chans = stream_channels()
    fb = eng.frame_bytes
    res = {"range": np.array([halo, begin, end])}
    keep = []

    def ios_for(a, z, frames):
        piece = torch.from_numpy(pack_layout([c[a:z] for c in chans], "I", 1)).to(dev)
        out_t = torch.zeros((frames * fb + 31) // 16 * 16, dtype=torch.uint8, device=dev)
        keep.extend([piece, out_t])
        ios = (d.FileIO * 1)()
        ios[0].dsd = piece.data_ptr(); ios[0].bytes_per_channel = z - a
        ios[0].pcm = out_t.data_ptr(); ios[0].pcm_capacity_bytes = frames * fb
        return ios, out_t

    pcm = []
    if end > begin:
        eng.seek(halo)
        if begin > halo:
            ios, _ = ios_for(halo, begin, 0)
            eng.prime_batch_device(ios)
        mid = begin + (end - begin) // 2 + 1                   # (an odd split: the second call starts off the stage-A grid)
        for a, z in ((begin, mid), (mid, end)):
            ios, out_t = ios_for(a, z, eng.next_frames(z - a))
            eng.translate_batch_device(ios)
            torch.cuda.synchronize()
            pcm.append(out_t[:ios[0].frames_out * fb].cpu().numpy().copy())
        assert eng.tell()[0] == end
    res["pcm"] = np.concatenate(pcm) if pcm else np.zeros(0, dtype=np.uint8)
    res["peaks"] = np.array([eng.peak(c) for c in range(CHN)])
    res["kernel"] = np.array(eng.kernel_name())
    np.savez(out, **res)
    eng.close()


if __name__ == "__main__":
    main()
