"""Measures what profiles/album_check.md reports, in one GPU session:

1. ALBUM AGAINST TRACKS.  N tracks of T seconds, DSD64 -> 88.2 kHz stereo 24-bit TPDF, verify + MD5 + loudness + true peak, at efforts
   0, 1 and 12: one d2d_convert_streams_flac on an engine of N files against N d2d_convert_stream_flac_loud calls one after another on
   an engine of one file (created once, reset between tracks).  The same at N = 1.  Both sides read from memory and throw the
   frames away through the same Python callbacks; a window is a host clock around calls that end in a device synchronise.
2. THE SEGMENT KERNELS AGAINST THE COPIES THEY REPLACE.  The driver's segment list of one chunk of a 64-file batch (per file: the
   carried frames and the new frames behind them, for the encoder's and for the meter's buffer; the frame bytes of every file to pinned
   memory) through d2d_segments_move_device + d2d_segments_pack_device, against the same bytes as hipMemcpyAsync calls with the
   synchronise a host needs before it knows the lengths.  Host time to enqueue, and time until the synchronise returns.

The two sides of each comparison alternate, after a warm-up of both.  usage: python tools/album_check.py [--tracks 16] [--seconds 60]
[--rounds 3] [--out bench_out/album_check.md]"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

KW = dict(dsd_rate=1, output_rate=88200, channels=2, fmt="P", endianness="L", block_size=4096, filter="E", bit_depth=24, dither="T", seed=1)


def reader(data, ch=2):
    pos = [0]

    def read(cap):
        a = pos[0]
        pos[0] = min(len(data), a + cap * ch)
        return data[a:pos[0]]
    return read


def drop(_):
    pass


def spread(xs):
    return f"{statistics.median(xs):.3f} s (min {min(xs):.3f}, max {max(xs):.3f}, n = {len(xs)})"


def album_against_tracks(d, data, n, effort, rounds, lines):
    import torch
    total = len(data) // 2
    batch = d.Engine(n_files=n, **KW)
    single = d.Engine(**KW)

    def album():
        batch.reset()
        meters = [d.LoudMeter(2, 88200, true_peak=True) for _ in range(n)]
        torch.cuda.synchronize()
        t = time.perf_counter()
        r = batch.convert_streams_flac([reader(data) for _ in range(n)], [drop] * n, totals=[total] * n, effort=effort, verify=True, md5=True, louds=meters)
        torch.cuda.synchronize()
        t = time.perf_counter() - t
        return t, r["md5"][0], bytes(meters[n - 1].finish()), r

    def tracks():
        meters = [d.LoudMeter(2, 88200, true_peak=True) for _ in range(n)]
        torch.cuda.synchronize()
        t = time.perf_counter()
        for f in range(n):
            single.reset()
            _, _, md5 = single.convert_stream_flac(reader(data), drop, total_bytes_per_channel=total, effort=effort, verify=True, md5=True, loud=meters[f])
        torch.cuda.synchronize()
        t = time.perf_counter() - t
        return t, md5, bytes(meters[n - 1].finish())

    a, b = album(), tracks()                                        # warm-up of both sides, and the results must not differ
    assert a[1] == b[1] and a[2] == b[2], "album and tracks disagree"
    ta, tb = [], []
    for _ in range(rounds):
        ta.append(album()[0])
        tb.append(tracks()[0])
    r = a[3]
    lines.append(f"| {n} | {effort} | {spread(ta)} | {spread(tb)} | {statistics.median(tb) / statistics.median(ta):.2f} | {r['chunks']} | {r['device_calls']} |")
    print(lines[-1], flush=True)
    batch.close(); single.close()


def segments_against_copies(d, rounds, lines, files=64):
    import torch
    try:
        hip = C.CDLL("libamdhip64.so.7")                             # by soname: the runtime torch has loaded
    except OSError:
        hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    D2D, D2H = 3, 2
    fb, nf, carry, kept = 6, (1 << 19) * 8 // 32, 2931, 2 * 8820 + 5000           # a 512 KiB chunk of stereo DSD64: 131072 new frames
    frame_bytes = 470000                                                         # of one file's chunk, about 60 % of its PCM
    slot = (carry + nf + kept + 4096) * fb // 16 * 16
    new = torch.randint(0, 255, (files * slot,), dtype=torch.uint8, device="cuda")
    pcm = [torch.zeros(files * slot, dtype=torch.uint8, device="cuda") for _ in range(2)]
    loud = [torch.zeros(files * slot, dtype=torch.uint8, device="cuda") for _ in range(2)]
    out = torch.randint(0, 255, (files * slot,), dtype=torch.uint8, device="cuda")
    lens = torch.full((files,), frame_bytes, dtype=torch.int64).pin_memory()
    h_out = torch.zeros(files * slot, dtype=torch.uint8).pin_memory()
    table = torch.zeros(files + 1, dtype=torch.int64).pin_memory()
    segs = (d.Segment * (4 * files))()
    for f in range(files):
        o = f * slot
        segs[4 * f + 0] = d.Segment(pcm[1].data_ptr() + o, pcm[0].data_ptr() + o + 4096 * fb, carry * fb)
        segs[4 * f + 1] = d.Segment(pcm[1].data_ptr() + o + carry * fb, new.data_ptr() + o, nf * fb)
        segs[4 * f + 2] = d.Segment(loud[1].data_ptr() + o, loud[0].data_ptr() + o + 3000 * fb, kept * fb)
        segs[4 * f + 3] = d.Segment(loud[1].data_ptr() + o + kept * fb, new.data_ptr() + o, nf * fb)
    srcs = (d.PackSrc * files)()
    for f in range(files):
        srcs[f] = d.PackSrc(out.data_ptr() + f * slot, lens.data_ptr() + 8 * f, frame_bytes + 4096)

    h_base, bases = h_out.data_ptr(), [s.base for s in srcs]

    def kernels():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        d.segments_move_device(segs)
        d.segments_pack_device(srcs, h_out.data_ptr(), files * slot, table.data_ptr())
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        return t1 - t0, time.perf_counter() - t0

    def copies():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for s in segs:
            hip.hipMemcpyAsync(s.dst, s.src, s.bytes, D2D, None)
        t1 = time.perf_counter()
        torch.cuda.synchronize()                                    # the lengths are the device's: a host that copies must wait for them
        t2 = time.perf_counter()
        at = 0
        for f, n in enumerate(lens.tolist()):
            hip.hipMemcpyAsync(h_base + at, bases[f], n, D2H, None)
            at += n
        t3 = time.perf_counter()
        torch.cuda.synchronize()
        return (t1 - t0) + (t3 - t2), time.perf_counter() - t0

    kernels(); copies(); kernels(); copies()
    want = h_out[:files * frame_bytes].clone()
    kernels()
    assert torch.equal(h_out[:files * frame_bytes], want) and int(table[files]) == files * frame_bytes, "the two forms disagree"
    k, c = [], []
    for _ in range(rounds * 5):
        k.append(kernels())
        c.append(copies())
    moved = sum(s.bytes for s in segs) + files * frame_bytes

    def us(xs):
        xs = [x * 1e6 for x in xs]
        return f"{statistics.median(xs):.0f} us (min {min(xs):.0f}, max {max(xs):.0f})"
    lines.append(f"| move + pack kernels | {us([x[0] for x in k])} | {us([x[1] for x in k])} |")
    lines.append(f"| {4 * files} + {files} hipMemcpyAsync, one more synchronise | {us([x[0] for x in c])} | {us([x[1] for x in c])} |")
    lines.append("")
    lines.append(f"{files} files, {moved / 1e6:.1f} MB per chunk ({len(k)} alternated rounds); the kernels reach "
                 f"{moved / statistics.median([x[1] for x in k]) / 1e9:.0f} GB/s of copied bytes to the synchronise.")
    print("\n".join(lines[-4:]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tracks", type=int, default=16)
    ap.add_argument("--seconds", type=float, default=60.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--efforts", default="0,1,12")
    ap.add_argument("--out", default=os.path.join(ROOT, "bench_out", "album_check.md"))
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "album_check needs a GPU: nothing here is measured without one"
    import dsd2dxd_amd as d
    from helpers import pack_layout, synth
    per_channel = int(a.seconds * 352800) // 4096 * 4096
    data = pack_layout([synth("sine", per_channel, seed=1), synth("pink", per_channel, seed=2, amp=0.098)], "P", 4096).tobytes()
    lines = [f"## Album against tracks: {a.tracks} tracks of {a.seconds:g} s, DSD64 -> 88.2 kHz stereo 24-bit, verify + MD5 + loudness + true peak", "",
             "| files | effort | one d2d_convert_streams_flac | d2d_convert_stream_flac_loud, one after another | tracks / album | chunks | device calls |",
             "|---|---|---|---|---|---|---|"]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)

    def save():
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    seg = ["", "## The segment kernels against the copies they replace", "", "| form | host time to enqueue | to the synchronise |", "|---|---|---|"]
    segments_against_copies(d, a.rounds, seg)
    for effort in [int(x) for x in a.efforts.split(",")]:
        for n in (a.tracks, 1):
            album_against_tracks(d, data, n, effort, a.rounds, lines)
            save()
    lines += seg
    save()
    print("\n".join(lines))


if __name__ == "__main__":
    main()
