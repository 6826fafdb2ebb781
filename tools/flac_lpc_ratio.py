#!/usr/bin/env python3
"""What does FLAC effort 12 save over effort 1 on converter output, counted on the CPU?
   tools/flac_lpc_ratio.py [seconds]        (no GPU; default 3 s per signal)

Synthetic DSD64 (sines; pink noise, as the bench batch mixes them) goes through the CPU oracle to 24-bit 88.2 kHz TPDF stereo, and
d2d_flac_encode_host_effort encodes it block by block at efforts 0, 1 and 12.  Printed per material: bytes, effort 12 over effort 1,
the worst frame's ratio and which LPC orders the frames' subframes carry.  A frame longer at effort 12 than at effort 1 is a bug by
rule 17 of csrc/flac/flac_frame_enc.h and fails the run.  The GPU encodes the same bytes (tests/test_gpu_flac_lpc.py), so these
ratios are the ones to hold tools/flac_probe.py --effort 12 against."""
import os
import sys
from collections import Counter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import dsd2dxd_amd as d
import flac_lpc_ref as P
from helpers import pack_layout, synth
from oracle import oracle as O

seconds = float(sys.argv[1]) if len(sys.argv) > 1 else 3.0
nbytes = max(1, int(round(seconds * 2822400 / 8 / 4096))) * 4096
KW = dict(dsd_rate=1, output_rate=88200, channels=2, fmt="P", endianness="L", block_size=4096, filter="E", bit_depth=24, dither="T", seed=206)
MATERIAL = {"sines": [synth("sine", nbytes, seed=1), synth("sine", nbytes, seed=2, amp=0.3)],
            "pink noise": [synth("pink", nbytes, seed=3, amp=0.098), synth("pink", nbytes, seed=4, amp=0.098)]}
for name, chans in MATERIAL.items():
    pcm, frames = O.Oracle(**KW).translate(pack_layout(chans, "P", 4096))
    sizes = {}
    for effort in (0, 1, 12):
        data = d.flac_encode_host(2, 24, pcm[:frames * 6], first_block=0, final=True, effort=effort)[0]
        _, sizes[effort], infos = P.decode(data, 2, 24)
    assert all(a <= b <= c for a, b, c in zip(sizes[12], sizes[1], sizes[0])), "a frame grew with the effort"
    kinds = Counter("%s %d" % (kind, order) for _, subs in infos for kind, order, _ in subs)
    print("%s: %d frames of 88.2 kHz stereo in %d blocks; bytes at efforts 0 / 1 / 12: %d / %d / %d; 12 over 1: %.4f (worst frame %.4f); 1 over 0: %.4f; subframes: %s" %
          (name, frames, len(sizes[0]), sum(sizes[0]), sum(sizes[1]), sum(sizes[12]), sum(sizes[12]) / sum(sizes[1]),
           max(a / b for a, b in zip(sizes[12], sizes[1])), sum(sizes[1]) / sum(sizes[0]), dict(kinds)))
