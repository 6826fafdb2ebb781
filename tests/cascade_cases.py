"""The two-stage 48 kHz definition (filter 'S', include/dsd2dxd_amd.h): the cases, inputs and oracle runs that tests/golden/make_cascade_golden.py,
tests/test_cascade_cpu.py and tests/test_gpu_cascade.py share.

The expected bytes come from the CPU oracle in its cascade mode (Oracle(filter="E").use_cascade(): stage A to 352.8 kHz on its integer grid, stage B
polyphase L/147 on its own).  The oracle knows the definition as a mode, not as a filter letter, so `oracle_kw` turns an engine's parameters into the
oracle's."""
import hashlib

import numpy as np

from helpers import pack_layout, random_bytes, synth

# the rate pairs filter 'E' serves with a composed one-pass table: under 'S' they are the cascade, other bytes
COMPOSED = [(1, 96000), (1, 192000), (1, 384000), (2, 96000), (2, 192000), (2, 384000), (4, 192000), (4, 384000)]
# ... and the pairs that are the cascade under 'E' already: 'S' gives the same bytes
CONTROL = [(4, 96000), (8, 96000)]

# Bytes per channel per call at DSD64 (times dsd_rate at the higher rates): one byte is one stage-A sample there, 147 of them one L/147 cycle, and
# stage B's tile is eight cycles (stereo: 1176 samples).  The first call holds a single sample; calls end mid-cycle, just below, at and just above a
# tile; the last one is several tiles and a remainder.
RAGGED = (1, 146, 147, 1175, 1176, 1177, 4096 + 13)
PLANAR = (4096, 8192, 4096)

IL = dict(fmt="I", endianness="M", block_size=1)            # byte-interleaved, MSB first: a DFF file's layout
PL = dict(fmt="P", endianness="L", block_size=4096)         # planar blocks, LSB first: a DSF file's layout


def ragged_calls(dsd_rate):
    return [n * dsd_rate for n in RAGGED]


def pair_id(dsd_rate, rate):
    return "dsd%d_%dk" % (64 * dsd_rate, rate // 1000)


def recipe_for(channels, nbytes, dsd_rate, msb_first, base):
    """what every channel holds: a sine, pink noise or random bytes in turn, each with a seed of its own"""
    rec = []
    for c in range(channels):
        if c % 3 == 0:
            rec.append(dict(kind="sine", seed=base + c, amp=0.352, freq=1000.0 + 111 * c))
        elif c % 3 == 1:
            rec.append(dict(kind="pink", seed=base + 100 + c, amp=0.098, freq=1000.0))
        else:
            rec.append(dict(kind="random", seed=base + 200 + c))
    return dict(nbytes=nbytes, dsd_rate=dsd_rate, msb_first=bool(msb_first), channels=rec)


def make_channels(recipe):
    out = []
    for ch in recipe["channels"]:
        if ch["kind"] == "random":
            out.append(random_bytes(recipe["nbytes"], ch["seed"]))
        else:
            out.append(synth(ch["kind"], recipe["nbytes"], seed=ch["seed"], amp=ch["amp"], freq=ch["freq"], dsd_rate=recipe["dsd_rate"],
                             msb_first=recipe["msb_first"]))
    return out


def call_buffers(chans, calls, fmt, block_size):
    """the channels cut into consecutive calls of `calls` bytes per channel, each in the engine's layout"""
    bufs, at = [], 0
    for n in calls:
        bufs.append(pack_layout([c[at:at + n] for c in chans], fmt, block_size))
        at += n
    assert at <= len(chans[0])
    return bufs


def oracle_kw(kw):
    """an 'S' engine's parameters as the oracle takes them (the caller adds use_cascade())"""
    drop = ("kernel", "channel_first", "channel_count", "debug", "device", "tap_bits")
    return dict({k: v for k, v in kw.items() if k not in drop}, filter="E")


def oracle_run(O, kw, bufs, cascade=True):
    """the oracle's conversion of the calls: (PCM of all calls as one uint8 array, frames per call, peak per channel)"""
    o = O.Oracle(**oracle_kw(kw))
    if cascade:
        o.use_cascade()
    parts, frames = [], []
    for b in bufs:
        pcm, fr = o.translate(b)
        parts.append(pcm[:fr * o.frame_bytes].copy())
        frames.append(int(fr))
    peaks = [o.peak(c) for c in range(kw["channels"])]
    o.close()
    return np.concatenate(parts) if parts else np.zeros(0, np.uint8), frames, peaks


def golden_cases():
    """name -> (engine parameters without the filter letter, calls, input recipe): what tests/golden/cascade_digests.json pins"""
    cases = {}
    for i, (dr, rate) in enumerate(COMPOSED + CONTROL):
        s24 = dict(dsd_rate=dr, output_rate=rate, channels=2, bit_depth=24, dither="T", seed=40 + i)
        calls = ragged_calls(dr)
        cases[pair_id(dr, rate) + "_s24_tpdf_ragged"] = (dict(s24, **IL), calls, recipe_for(2, sum(calls), dr, True, 1000 + 10 * i))
        cases[pair_id(dr, rate) + "_s24_tpdf_planar"] = (dict(s24, **PL), list(PLANAR), recipe_for(2, sum(PLANAR), dr, False, 2000 + 10 * i))
    calls = ragged_calls(1)
    cases["dsd64_192k_f32_fpd_m3db"] = (dict(dsd_rate=1, output_rate=192000, channels=2, bit_depth=32, dither="F", level_db=-3.0, seed=61, **IL), calls,
                                         recipe_for(2, sum(calls), 1, True, 3000))
    cases["dsd128_96k_s24_ns"] = (dict(dsd_rate=2, output_rate=96000, channels=2, bit_depth=24, dither="N", seed=62, **PL), list(PLANAR),
                                   recipe_for(2, sum(PLANAR), 2, False, 3100))
    cases["dsd64_96k_6ch_s16_tpdf"] = (dict(dsd_rate=1, output_rate=96000, channels=6, bit_depth=16, dither="T", seed=63, **PL), list(PLANAR),
                                        recipe_for(6, sum(PLANAR), 1, False, 3200))
    return cases


def digest_entry(O, kw, calls, recipe):
    """one entry of cascade_digests.json, computed by the oracle in cascade mode"""
    bufs = call_buffers(make_channels(recipe), calls, kw["fmt"], kw["block_size"])
    pcm, frames, peaks = oracle_run(O, kw, bufs)
    fb = len(pcm) // max(sum(frames), 1)
    return dict(kw=kw, calls=list(calls), input=recipe, frames=frames, sha256=hashlib.sha256(pcm.tobytes()).hexdigest(),
                head=pcm[:32 * fb].tobytes().hex(), peaks=peaks)
