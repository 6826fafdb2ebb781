#!/usr/bin/env python3
"""What does encoding the bench batch's PCM to FLAC cost on the GPU, beside the 16 host threads the sink uses and beside the conversion?
   tools/flac_probe.py [--effort N] [files] [seconds] [reps] [out.json]
   (needs the GPU; defaults effort 0, 64 files, 60 s each, 9 repetitions, bench_out/flac_probe.json)

The PCM is what d2d_translate_batch_device writes for the bench shape (distinct DSD64 stereo files -> 24-bit 88.2 kHz, TPDF): real
converter output.  GPU figure: device events around ONE d2d_flac_encode_device call over the whole batch (both kernels), after warm-ups,
median of the repetitions; the conversion step is timed the same way on the same batch.  Baseline: d2d_flac_encode_host -- the sink's
own encoder -- on the same PCM in host memory, one block per task on 16 threads, as FlacSink::drain spreads them; wall clock, best of
two passes.  File 0's device frames are compared with the host's.  With --effort 1 (the search, D2D_FLAC_EFFORT_SEARCH) both sides run
at that effort, and the effort-0 call is timed beside it on the same buffers for the size ratio.  With --effort 12 (the search with
LPC, D2D_FLAC_EFFORT_LPC) the call timed beside it is effort 1's, in the same session on the same buffers: bytes and time are stated
over effort 1's, and no file may come out longer than at effort 1.

   tools/flac_probe.py --verify [--method serial|coop] [files] [seconds] [reps] [out.json]      (default bench_out/flac_verify_probe.json)
times ONE d2d_flac_verify_device_method call over the batch (both kernels) at each effort, after that effort's encode call on the same
buffers, beside the encode call itself; every record must be clean.  The ratio verify / encode at the same effort is the figure of
interest.  --method chooses D2D_FLAC_VERIFY_SERIAL (one lane per frame) or D2D_FLAC_VERIFY_COOP (one workgroup per frame); without it
the call is AUTO's.  Under coop every block must have been accepted by the fast path.

   tools/flac_probe.py --md5 [files] [seconds] [reps] [out.json]                                (default bench_out/flac_md5_probe.json)
STREAMINFO's MD5 on the device, all in one session on the batch's PCM: (a) ONE d2d_flac_md5_update_device call over the whole batch,
device events, ms and GB/s per file; (b) the same call over one file; (c) the encode call at efforts 0 / 1 / 12 beside it, and the update
on a second stream beside the effort-12 encode (first event to last event: does it hide?); (d) what a caller has without the call: the
batch's PCM copied to pinned host memory (events) and hashed there on 16 threads, one file per task (wall clock), by the host twin
d2d_flac_md5_update_host and by hashlib (OpenSSL).  Every file's device digest must be hashlib's.

   tools/flac_probe.py --loud [files] [seconds] [reps] [out.json]                               (default bench_out/loud_probe.json)
Loudness cells on the device, all in one session on the batch's PCM: (a) ONE d2d_loud_measure_device call over the whole batch, device
events; (b) the same call over one file; (c) the encode call at efforts 0 / 1 / 12 beside it, and the measure call on a second stream
beside the effort-12 encode; (d) the alternative: the batch's PCM copied to pinned host memory and measured there on 16 threads, one
file per task, by the CPU twin d2d_loud_measure_host; (e) the CLI's single-file case: one call over one chunk (4 MiB of DSD per
channel) of one file, a few waves whose lanes each walk 3 S frames.  Every file's device cells must be the CPU twin's bytes.

   tools/flac_probe.py --true-peak [files] [seconds] [reps] [out.json]                          (default bench_out/true_peak_probe.json)
True-peak doubles on the device, all in one session on the batch's PCM, each beside the loudness call measured again in the same session:
(a) ONE d2d_true_peak_measure_device call over the whole batch; (b) over one file; (e) over one chunk of one file; a device-to-device copy
of the same PCM, the memory floor; (c) the encode call at efforts 0 / 1 / 12, and the true-peak call on a second stream beside the
effort-12 encode; (d) the batch's PCM copied to pinned host memory and measured there on 16 threads by the CPU twin
d2d_true_peak_measure_host.  Every file's device doubles must be the CPU twin's bytes."""
import ctypes as C
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import dsd2dxd_amd as d
from bench import make_files, DSD64

argv = sys.argv[1:]
effort = 0
if "--effort" in argv:
    at = argv.index("--effort")
    effort = int(argv[at + 1])
    del argv[at:at + 2]
verify_mode = "--verify" in argv
if verify_mode:
    argv.remove("--verify")
md5_mode = "--md5" in argv
if md5_mode:
    argv.remove("--md5")
loud_mode = "--loud" in argv
if loud_mode:
    argv.remove("--loud")
tpeak_mode = "--true-peak" in argv
if tpeak_mode:
    argv.remove("--true-peak")
method_name = "auto"
if "--method" in argv:
    at = argv.index("--method")
    method_name = argv[at + 1]
    del argv[at:at + 2]
n_files = int(argv[0]) if len(argv) > 0 else 64
seconds = float(argv[1]) if len(argv) > 1 else 60.0
reps = int(argv[2]) if len(argv) > 2 else 9
out_path = argv[3] if len(argv) > 3 else os.path.join(ROOT, "bench_out", "true_peak_probe.json" if tpeak_mode else "loud_probe.json" if loud_mode else "flac_md5_probe.json" if md5_mode else "flac_verify_probe.json" if verify_mode else "flac_probe.json")
blocks_in = max(1, int(round(seconds * DSD64 / 8 / 4096)))
bpc = blocks_in * 4096
CH, DEPTH, BS, THREADS = 2, 24, 4096, 16
kw = dict(dsd_rate=1, output_rate=88200, channels=CH, fmt="P", endianness="L", block_size=4096, filter="E", bit_depth=DEPTH, dither="T", seed=206)
assert torch.cuda.is_available(), "flac_probe.py measures on the GPU; there is no other path"
dev = torch.device("cuda", 0)
stream = torch.cuda.current_stream().cuda_stream
L = d.lib()


def timed(fn, before=None):
    ms = []
    for i in range(3 + reps):
        if before:
            before()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if i >= 3:
            ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


# ---- the conversion step: the batch's PCM, device-resident
files = make_files(n_files, bpc, 1, n_files, 0, 16)
eng = d.Engine(n_files=n_files, kernel=d.KERNEL_AUTO, device=0, **kw)
frames, fb = eng.next_frames(bpc), eng.frame_bytes
ins = [torch.from_numpy(b).to(dev) for b in files]
row = (frames * fb + 31) // 16 * 16
pcm = torch.empty((n_files, row), dtype=torch.uint8, device=dev)
tio = (d.FileIO * n_files)()
for f in range(n_files):
    tio[f].dsd, tio[f].bytes_per_channel, tio[f].pcm, tio[f].pcm_capacity_bytes = ins[f].data_ptr(), bpc, pcm[f].data_ptr(), frames * fb
conv = timed(lambda: eng.translate_batch_device(tio, stream), before=eng.reset)

# ---- the encode call
cap = d.flac_bound_bytes(CH, DEPTH, frames, True)
cap16 = (cap + 15) // 16 * 16
wsb = d.flac_workspace_bytes(CH, DEPTH, frames, True)
out = torch.empty((n_files, cap16), dtype=torch.uint8, device=dev)
ws = torch.empty(n_files * wsb, dtype=torch.uint8, device=dev)
rec = torch.zeros(n_files * 16, dtype=torch.uint8, device=dev)
fio = (d.FlacIO * n_files)()
for f in range(n_files):
    fio[f].pcm, fio[f].frames, fio[f].first_block, fio[f].final = pcm[f].data_ptr(), frames, 0, 1
    fio[f].out, fio[f].out_capacity_bytes, fio[f].result = out[f].data_ptr(), cap, rec.data_ptr() + 16 * f
if verify_mode:
    method = dict(auto=d.FLAC_VERIFY_AUTO, serial=d.FLAC_VERIFY_SERIAL, coop=d.FLAC_VERIFY_COOP)[method_name]
    chk = torch.zeros(n_files * 24, dtype=torch.uint8, device=dev)
    vst = torch.zeros(n_files * 8, dtype=torch.uint8, device=dev)
    res = dict(files=n_files, seconds_per_file=seconds, frames_per_file=frames, reps=reps, method=method_name, efforts={})
    print("batch: %d files x %d frames, stereo 24-bit; verify method %s" % (n_files, frames, method_name))
    for eff in (d.FLAC_EFFORT_FIXED2, d.FLAC_EFFORT_SEARCH, d.FLAC_EFFORT_LPC):
        e_ms = timed(lambda: d.flac_encode_device(CH, DEPTH, fio, ws.data_ptr(), ws.numel(), stream, effort=eff))
        v_ms = timed(lambda: d.flac_verify_device(CH, DEPTH, fio, ws.data_ptr(), ws.numel(), chk.data_ptr(), stream, method=method, stats_ptr=vst.data_ptr()))
        c = chk.cpu().numpy()
        fast = vst.cpu().numpy().view(np.uint32).reshape(n_files, 2)
        assert (fast[:, 0] == (0 if method_name == "serial" else int(fio[0].blocks))).all() and (fast.sum(axis=1) == int(fio[0].blocks)).all(), fast
        for f in range(n_files):
            r = c[24 * f:24 * f + 24]
            got = (int(r[:8].view(np.uint64)[0]),) + tuple(int(v) for v in r[8:].view(np.uint32))
            assert got == (frames, int(fio[f].blocks), 0, 0xFFFFFFFF, 0), (eff, f, got)
        res["efforts"][str(eff)] = dict(gpu_encode_ms=dict(median=e_ms[0], min=e_ms[1], max=e_ms[2]), gpu_verify_ms=dict(median=v_ms[0], min=v_ms[1], max=v_ms[2]),
                                        verify_over_encode=v_ms[0] / e_ms[0], blocks=n_files * int(fio[0].blocks))
        print("effort %2d: encode median %.3f ms (min %.3f, max %.3f); verify median %.3f ms (min %.3f, max %.3f); verify / encode %.2fx; %d blocks, all good" %
              (eff, *e_ms, *v_ms, v_ms[0] / e_ms[0], n_files * int(fio[0].blocks)))
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        json.dump(res, fh, indent=1)
    sys.exit(0)
if md5_mode:
    import hashlib
    states = torch.zeros(n_files * 96, dtype=torch.uint8, device=dev)
    digests = torch.zeros(n_files * 16, dtype=torch.uint8, device=dev)
    mio = (d.FlacMd5IO * n_files)()
    for f in range(n_files):
        mio[f].pcm, mio[f].frames = pcm[f].data_ptr(), frames
    one = (d.FlacMd5IO * 1)()
    one[0].pcm, one[0].frames = pcm[0].data_ptr(), frames
    file_bytes = frames * fb
    fresh = lambda: d.flac_md5_init_device(states.data_ptr(), n_files, stream)
    ms3 = lambda t: dict(median=t[0], min=t[1], max=t[2])
    # (a), (b)
    batch_ms = timed(lambda: d.flac_md5_update_device(CH, DEPTH, mio, states.data_ptr(), stream), before=fresh)
    d.flac_md5_final_device(states.data_ptr(), n_files, digests.data_ptr(), stream)
    got = digests.cpu().numpy().tobytes()
    one_ms = timed(lambda: d.flac_md5_update_device(CH, DEPTH, one, states.data_ptr(), stream), before=fresh)
    # (c)
    enc_ms = {eff: timed(lambda: d.flac_encode_device(CH, DEPTH, fio, ws.data_ptr(), ws.numel(), stream, effort=eff)) for eff in (0, 1, 12)}
    s_enc, s_md5 = torch.cuda.Stream(), torch.cuda.Stream()

    def beside():
        ms = []
        for i in range(3 + reps):
            fresh()
            torch.cuda.synchronize()
            a, b1, b2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
            a.record()
            s_enc.wait_event(a)
            s_md5.wait_event(a)
            d.flac_md5_update_device(CH, DEPTH, mio, states.data_ptr(), s_md5.cuda_stream)
            d.flac_encode_device(CH, DEPTH, fio, ws.data_ptr(), ws.numel(), s_enc.cuda_stream, effort=12)
            b1.record(s_enc)
            b2.record(s_md5)
            torch.cuda.synchronize()
            if i >= 3:
                ms.append((max(a.elapsed_time(b1), a.elapsed_time(b2)), a.elapsed_time(b1), a.elapsed_time(b2)))
        return [statistics.median(m[k] for m in ms) for k in range(3)]

    both_ms = beside()
    # (d)
    pinned = torch.empty((n_files, file_bytes), dtype=torch.uint8).pin_memory()
    copy_ms = timed(lambda: [pinned[f].copy_(pcm[f, :file_bytes], non_blocking=True) for f in range(n_files)])      # (one contiguous copy per file)
    host_pcm = pinned.numpy()
    want = [hashlib.md5(host_pcm[f]).digest() for f in range(n_files)]
    assert [got[16 * f:16 * f + 16] for f in range(n_files)] == want, "a device digest is not hashlib's"

    def twin(f):
        st = d.flac_md5_init_host(1)
        d.flac_md5_update_host(CH, DEPTH, host_pcm[f], st[0])
        return d.flac_md5_final_host(st[0])

    host = {}
    with ThreadPoolExecutor(THREADS) as pool:
        for name, fn in (("host_twin", twin), ("hashlib", lambda f: hashlib.md5(host_pcm[f]).digest())):
            s = []
            for _ in range(2):
                t0 = time.perf_counter()
                assert list(pool.map(fn, range(n_files))) == want
                s.append(time.perf_counter() - t0)
            host[name] = s
    gbs = lambda ms: file_bytes / ms / 1e6
    res = dict(files=n_files, seconds_per_file=seconds, frames_per_file=frames, bytes_per_file=file_bytes, reps=reps,
               update_batch_ms=ms3(batch_ms), update_one_file_ms=ms3(one_ms), gb_per_s_per_file_batch=gbs(batch_ms[0]), gb_per_s_one_file=gbs(one_ms[0]),
               encode_ms={str(k): ms3(v) for k, v in enc_ms.items()}, conversion_ms=ms3(conv),
               beside_effort12_ms=dict(first_to_last=both_ms[0], encode_end=both_ms[1], update_end=both_ms[2]),
               copy_to_pinned_ms=ms3(copy_ms), host_16_threads_s=host, digests_equal_hashlib=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        json.dump(res, fh, indent=1)
    print("batch: %d files x %d frames, stereo 24-bit: %.2f MB per file; every device digest equals hashlib's" % (n_files, frames, file_bytes / 1e6))
    print("(a) update, whole batch, one call: median %.2f ms (min %.2f, max %.2f) = %.4f GB/s per file, %.3f GB/s in all" %
          (*batch_ms, gbs(batch_ms[0]), n_files * gbs(batch_ms[0])))
    print("(b) update, one file:              median %.2f ms (min %.2f, max %.2f) = %.4f GB/s" % (*one_ms, gbs(one_ms[0])))
    for eff in (0, 1, 12):
        print("(c) encode effort %2d alone: median %.2f ms (min %.2f, max %.2f)" % (eff, *enc_ms[eff]))
    print("(c) conversion step alone: median %.2f ms" % conv[0])
    print("(c) update on a second stream beside the effort-12 encode: first event to last %.2f ms (encode ends at %.2f, update at %.2f)" % tuple(both_ms))
    print("(d) copy to pinned host memory: median %.2f ms (min %.2f, max %.2f) = %.1f GB/s" % (*copy_ms, n_files * file_bytes / copy_ms[0] / 1e6))
    for name, s in host.items():
        print("(d) %s on %d threads, one file per task: best %.3f s of %s" % (name, THREADS, min(s), ["%.3f" % v for v in s]))
    sys.exit(0)
if loud_mode:
    RATE, S = kw["output_rate"], kw["output_rate"] // 10
    rows = frames // S + 1
    cells = torch.zeros((n_files, rows * CH * 2), dtype=torch.float64, device=dev)
    file_bytes = frames * fb
    ms3 = lambda t: dict(median=t[0], min=t[1], max=t[2])

    def ios(n, nframes):
        x = (d.LoudIO * n)()
        for f in range(n):
            x[f] = d.LoudIO(pcm[f].data_ptr(), nframes, 0, 0, 1, 0, cells[f].data_ptr(), rows * CH, 0, 0, 0)
        return x

    lio, one = ios(n_files, frames), ios(1, frames)
    chunk_frames = min(frames, (4 << 20) * 8 // 32)                     # what 4 MiB of DSD64 per channel make at 88.2 kHz
    small = ios(1, chunk_frames)
    # (a), (b), (e)
    batch_ms = timed(lambda: d.loud_measure_device(CH, DEPTH, RATE, lio, stream))
    got = cells.cpu().numpy().copy()
    one_ms = timed(lambda: d.loud_measure_device(CH, DEPTH, RATE, one, stream))
    small_ms = timed(lambda: d.loud_measure_device(CH, DEPTH, RATE, small, stream))
    # (c)
    enc_ms = {eff: timed(lambda: d.flac_encode_device(CH, DEPTH, fio, ws.data_ptr(), ws.numel(), stream, effort=eff)) for eff in (0, 1, 12)}
    s_enc, s_loud = torch.cuda.Stream(), torch.cuda.Stream()

    def beside():
        ms = []
        for i in range(3 + reps):
            torch.cuda.synchronize()
            a, b1, b2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
            a.record()
            s_enc.wait_event(a)
            s_loud.wait_event(a)
            d.loud_measure_device(CH, DEPTH, RATE, lio, s_loud.cuda_stream)
            d.flac_encode_device(CH, DEPTH, fio, ws.data_ptr(), ws.numel(), s_enc.cuda_stream, effort=12)
            b1.record(s_enc)
            b2.record(s_loud)
            torch.cuda.synchronize()
            if i >= 3:
                ms.append((max(a.elapsed_time(b1), a.elapsed_time(b2)), a.elapsed_time(b1), a.elapsed_time(b2)))
        return [statistics.median(m[k] for m in ms) for k in range(3)]

    both_ms = beside()
    # (d)
    pinned = torch.empty((n_files, file_bytes), dtype=torch.uint8).pin_memory()
    copy_ms = timed(lambda: [pinned[f].copy_(pcm[f, :file_bytes], non_blocking=True) for f in range(n_files)])
    host_pcm = pinned.numpy()

    def twin(f):
        c, io = d.loud_measure_host(CH, DEPTH, RATE, host_pcm[f])
        return c.tobytes()

    with ThreadPoolExecutor(THREADS) as pool:
        t0 = time.perf_counter()
        want = list(pool.map(twin, range(n_files)))
        host_s = time.perf_counter() - t0
    n_cells = int(lio[0].cells_out)
    bad = [f for f in range(n_files) if got[f, :2 * n_cells].tobytes() != want[f]]
    assert not bad, "the device cells of files %s are not the CPU twin's bytes" % bad
    m = d.LoudMeter(CH, RATE)
    m.add(got[0, :2 * n_cells].reshape(-1, CH, 2), has_partial=n_cells > int(lio[0].subblocks) * CH)
    r0 = m.finish()
    units = n_cells
    res = dict(files=n_files, seconds_per_file=seconds, frames_per_file=frames, bytes_per_file=file_bytes, reps=reps, units_per_file=units,
               measure_batch_ms=ms3(batch_ms), measure_one_file_ms=ms3(one_ms), measure_one_chunk_ms=ms3(small_ms), chunk_frames=chunk_frames,
               encode_ms={str(k): ms3(v) for k, v in enc_ms.items()}, conversion_ms=ms3(conv),
               beside_effort12_ms=dict(first_to_last=both_ms[0], encode_end=both_ms[1], measure_end=both_ms[2]),
               copy_to_pinned_ms=ms3(copy_ms), host_twin_16_threads_s=host_s, cells_equal_host_twin=True, file0_lufs=r0.lufs, file0_peak=r0.peak)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        json.dump(res, fh, indent=1)
    gbs = lambda ms, n=1: n * file_bytes / ms / 1e6
    print("batch: %d files x %d frames, stereo 24-bit: %.2f MB per file, %d units (lanes) per file; every file's device cells are the CPU twin's bytes" %
          (n_files, frames, file_bytes / 1e6, units))
    print("file 0: %.3f LUFS, peak %.6f" % (r0.lufs, r0.peak))
    print("(a) measure, whole batch, one call: median %.3f ms (min %.3f, max %.3f) = %.2f GB/s of PCM" % (*batch_ms, gbs(batch_ms[0], n_files)))
    print("(b) measure, one file:              median %.3f ms (min %.3f, max %.3f) = %.2f GB/s" % (*one_ms, gbs(one_ms[0])))
    print("(e) measure, one chunk of one file (%d frames, %d lanes): median %.3f ms (min %.3f, max %.3f)" % (chunk_frames, chunk_frames // S * CH + CH, *small_ms))
    for eff in (0, 1, 12):
        print("(c) encode effort %2d alone: median %.2f ms (min %.2f, max %.2f)" % (eff, *enc_ms[eff]))
    print("(c) conversion step alone: median %.2f ms" % conv[0])
    print("(c) measure on a second stream beside the effort-12 encode: first event to last %.2f ms (encode ends at %.2f, measure at %.2f)" % tuple(both_ms))
    print("(d) copy to pinned host memory: median %.2f ms (min %.2f, max %.2f) = %.1f GB/s" % (*copy_ms, n_files * file_bytes / copy_ms[0] / 1e6))
    print("(d) CPU twin on %d threads, one file per task: %.3f s" % (THREADS, host_s))
    sys.exit(0)
if tpeak_mode:
    RATE, S = kw["output_rate"], kw["output_rate"] // 10
    rows = frames // S + 1
    peaks = torch.zeros((n_files, rows * CH), dtype=torch.float64, device=dev)
    cells = torch.zeros((n_files, rows * CH * 2), dtype=torch.float64, device=dev)
    file_bytes = frames * fb
    ms3 = lambda t: dict(median=t[0], min=t[1], max=t[2])

    def ios(kind, n, nframes):
        x = (kind * n)()
        for f in range(n):
            x[f] = kind(pcm[f].data_ptr(), nframes, 0, 0, 1, 0, (peaks if kind is d.TruePeakIO else cells)[f].data_ptr(), rows * CH, 0, 0, 0)
        return x

    chunk_frames = min(frames, (4 << 20) * 8 // 32)                     # what 4 MiB of DSD64 per channel make at 88.2 kHz
    pio, pone, psmall = ios(d.TruePeakIO, n_files, frames), ios(d.TruePeakIO, 1, frames), ios(d.TruePeakIO, 1, chunk_frames)
    lio, lone, lsmall = ios(d.LoudIO, n_files, frames), ios(d.LoudIO, 1, frames), ios(d.LoudIO, 1, chunk_frames)
    # (a), (b), (e): the true-peak call and, in the same session, the loudness call it accompanies
    tp_batch = timed(lambda: d.true_peak_measure_device(CH, DEPTH, RATE, pio, stream))
    got = peaks.cpu().numpy().copy()
    tp_one = timed(lambda: d.true_peak_measure_device(CH, DEPTH, RATE, pone, stream))
    tp_small = timed(lambda: d.true_peak_measure_device(CH, DEPTH, RATE, psmall, stream))
    ld_batch = timed(lambda: d.loud_measure_device(CH, DEPTH, RATE, lio, stream))
    ld_one = timed(lambda: d.loud_measure_device(CH, DEPTH, RATE, lone, stream))
    ld_small = timed(lambda: d.loud_measure_device(CH, DEPTH, RATE, lsmall, stream))
    # the memory floor: the same PCM copied device to device (it reads and writes: twice the traffic of a call that only reads)
    twin_pcm = torch.empty_like(pcm)
    d2d_ms = timed(lambda: twin_pcm.copy_(pcm))
    # (c)
    enc_ms = {eff: timed(lambda: d.flac_encode_device(CH, DEPTH, fio, ws.data_ptr(), ws.numel(), stream, effort=eff)) for eff in (0, 1, 12)}
    s_enc, s_tp = torch.cuda.Stream(), torch.cuda.Stream()

    def beside():
        ms = []
        for i in range(3 + reps):
            torch.cuda.synchronize()
            a, b1, b2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
            a.record()
            s_enc.wait_event(a)
            s_tp.wait_event(a)
            d.true_peak_measure_device(CH, DEPTH, RATE, pio, s_tp.cuda_stream)
            d.flac_encode_device(CH, DEPTH, fio, ws.data_ptr(), ws.numel(), s_enc.cuda_stream, effort=12)
            b1.record(s_enc)
            b2.record(s_tp)
            torch.cuda.synchronize()
            if i >= 3:
                ms.append((max(a.elapsed_time(b1), a.elapsed_time(b2)), a.elapsed_time(b1), a.elapsed_time(b2)))
        return [statistics.median(m[k] for m in ms) for k in range(3)]

    both_ms = beside()
    # (d)
    pinned = torch.empty((n_files, file_bytes), dtype=torch.uint8).pin_memory()
    copy_ms = timed(lambda: [pinned[f].copy_(pcm[f, :file_bytes], non_blocking=True) for f in range(n_files)])
    host_pcm = pinned.numpy()

    def twin(f):
        p, io = d.true_peak_measure_host(CH, DEPTH, RATE, host_pcm[f])
        return p.tobytes()

    with ThreadPoolExecutor(THREADS) as pool:
        t0 = time.perf_counter()
        want = list(pool.map(twin, range(n_files)))
        host_s = time.perf_counter() - t0
    n_out = int(pio[0].peaks_out)
    bad = [f for f in range(n_files) if got[f, :n_out].tobytes() != want[f]]
    assert not bad, "the device doubles of files %s are not the CPU twin's bytes" % bad
    sample0 = float(d.loud_measure_host(CH, DEPTH, RATE, host_pcm[0])[0][:, :, 1].max())
    res = dict(files=n_files, seconds_per_file=seconds, frames_per_file=frames, bytes_per_file=file_bytes, reps=reps, rows_per_file=n_out // CH,
               true_peak_batch_ms=ms3(tp_batch), true_peak_one_file_ms=ms3(tp_one), true_peak_one_chunk_ms=ms3(tp_small), chunk_frames=chunk_frames,
               loudness_batch_ms=ms3(ld_batch), loudness_one_file_ms=ms3(ld_one), loudness_one_chunk_ms=ms3(ld_small),
               device_to_device_copy_ms=ms3(d2d_ms), encode_ms={str(k): ms3(v) for k, v in enc_ms.items()}, conversion_ms=ms3(conv),
               beside_effort12_ms=dict(first_to_last=both_ms[0], encode_end=both_ms[1], measure_end=both_ms[2]),
               copy_to_pinned_ms=ms3(copy_ms), host_twin_16_threads_s=host_s, doubles_equal_host_twin=True,
               file0_true_peak=float(got[0, :n_out].max()), file0_sample_peak=sample0)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        json.dump(res, fh, indent=1)
    gbs = lambda ms, n=1: n * file_bytes / ms / 1e6
    print("batch: %d files x %d frames, stereo 24-bit: %.2f MB per file, %d rows (workgroups) per file; every file's device doubles are the CPU twin's bytes" %
          (n_files, frames, file_bytes / 1e6, n_out // CH))
    print("file 0: true peak %.6f, sample peak %.6f" % (res["file0_true_peak"], sample0))
    for name, tp, ld in (("(a) whole batch, one call", tp_batch, ld_batch), ("(b) one file", tp_one, ld_one), ("(e) one chunk of one file (%d frames)" % chunk_frames, tp_small, ld_small)):
        print("%s: true peak median %.3f ms (min %.3f, max %.3f); loudness median %.3f ms (min %.3f, max %.3f); true peak / loudness %.3f" % (name, *tp, *ld, tp[0] / ld[0]))
    print("(a) true peak over the batch = %.1f GB/s of PCM read; device-to-device copy of the same PCM: median %.3f ms (min %.3f, max %.3f) = %.1f GB/s read + as much written" %
          (gbs(tp_batch[0], n_files), *d2d_ms, n_files * pcm.shape[1] / d2d_ms[0] / 1e6))
    for eff in (0, 1, 12):
        print("(c) encode effort %2d alone: median %.2f ms (min %.2f, max %.2f); true peak / encode %.3f" % (eff, *enc_ms[eff], tp_batch[0] / enc_ms[eff][0]))
    print("(c) conversion step alone: median %.2f ms" % conv[0])
    print("(c) true peak on a second stream beside the effort-12 encode: first event to last %.2f ms (encode ends at %.2f, true peak at %.2f)" % tuple(both_ms))
    print("(d) copy to pinned host memory: median %.2f ms (min %.2f, max %.2f) = %.1f GB/s" % (*copy_ms, n_files * file_bytes / copy_ms[0] / 1e6))
    print("(d) CPU twin on %d threads, one file per task: %.3f s" % (THREADS, host_s))
    sys.exit(0)
enc0, bytes0, per_file0 = None, None, None
base = 1 if effort == d.FLAC_EFFORT_LPC else 0                  # the effort this one is held against
if effort:                                                      # the base effort on the same buffers first: its time and its bytes
    enc0 = timed(lambda: d.flac_encode_device(CH, DEPTH, fio, ws.data_ptr(), ws.numel(), stream, effort=base))
    per_file0 = rec.cpu().numpy().view(np.uint64).reshape(n_files, 2)[:, 0].copy()
    bytes0 = int(per_file0.sum())
enc = timed(lambda: d.flac_encode_device(CH, DEPTH, fio, ws.data_ptr(), ws.numel(), stream, effort=effort))
r = rec.cpu().numpy().view(np.uint64).reshape(n_files, 2)
flac_bytes = int(r[:, 0].sum())
nblocks = int(fio[0].blocks)

# ---- the baseline: the sink's encoder on 16 threads, one block per task
host_pcm = pcm[:, :frames * fb].cpu().numpy()
slot = d.flac_bound_bytes(CH, DEPTH, BS, True)
tls = {}


def one_block(job):
    f, b = job
    import threading
    st = tls.setdefault(threading.get_ident(), (np.empty(slot, dtype=np.uint8), d.FlacResult(), C.c_size_t()))
    n = min(BS, frames - b * BS)
    rc = L.d2d_flac_encode_host_effort(CH, DEPTH, effort, host_pcm[f].ctypes.data + b * BS * fb, n, b, 1, st[0].ctypes.data, slot, C.byref(st[1]), C.byref(st[2]))
    assert rc == 0
    return st[1].bytes_out


jobs = [(f, b) for f in range(n_files) for b in range(nblocks)]
host_s, host_bytes = [], 0
with ThreadPoolExecutor(THREADS) as pool:
    for _ in range(2):
        t0 = time.perf_counter()
        host_bytes = sum(pool.map(one_block, jobs, chunksize=64))
        host_s.append(time.perf_counter() - t0)
same_total = host_bytes == flac_bytes
want0, _, _ = d.flac_encode_host(CH, DEPTH, host_pcm[0], first_block=0, final=True, effort=effort)
same0 = out[0, :int(r[0, 0])].cpu().numpy().tobytes() == want0

pcm_bytes = n_files * frames * fb
res = dict(effort=effort, files=n_files, seconds_per_file=seconds, blocks_per_file=nblocks, frames_per_file=frames, pcm_bytes=pcm_bytes, flac_bytes=flac_bytes,
           ratio=flac_bytes / pcm_bytes, gpu_encode_ms=dict(median=enc[0], min=enc[1], max=enc[2]), conversion_ms=dict(median=conv[0], min=conv[1], max=conv[2]),
           host_16_threads_s=dict(best=min(host_s), passes=host_s), reps=reps, workspace_bytes=int(ws.numel()), crc="parallel (per-thread chunks, tree combine)",
           file0_equals_host=bool(same0), total_bytes_equal_host=bool(same_total), kernel=eng.kernel_name())
if effort:
    res.update({"base_effort": base, "effort%d_gpu_encode_ms" % base: dict(median=enc0[0], min=enc0[1], max=enc0[2]), "effort%d_flac_bytes" % base: bytes0,
                "size_over_effort%d" % base: flac_bytes / bytes0, "time_over_effort%d" % base: enc[0] / enc0[0],
                "worst_file_size_over_effort%d" % base: float((r[:, 0] / per_file0).max())})
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as fh:
    json.dump(res, fh, indent=1)
samples = n_files * frames * CH
print("batch: %d files x %d blocks (%d frames), PCM %.1f MB -> FLAC %.1f MB (ratio %.4f)" % (n_files, nblocks, frames, pcm_bytes / 1e6, flac_bytes / 1e6, flac_bytes / pcm_bytes))
print("effort %d" % effort)
if effort:
    print("effort %d on the same buffers: median %.3f ms (min %.3f, max %.3f), %.1f MB; effort %d / effort %d bytes: %.4f (worst file %.4f), time: %.2fx" %
          (base, *enc0, bytes0 / 1e6, effort, base, flac_bytes / bytes0, float((r[:, 0] / per_file0).max()), enc[0] / enc0[0]))
print("GPU encode (one d2d_flac_encode_device call, both kernels): median %.3f ms (min %.3f, max %.3f) = %.2f Gsamples/s" % (*enc, samples / enc[0] / 1e6))
print("conversion step (d2d_translate_batch_device, %s):  median %.3f ms (min %.3f, max %.3f)" % (eng.kernel_name(), *conv))
print("host, %d threads, one block per task: best %.3f s of %s = %.3f Gsamples/s" % (THREADS, min(host_s), ["%.3f" % s for s in host_s], samples / min(host_s) / 1e9))
print("GPU encode / host: %.1fx;  encode / conversion: %.2fx;  file 0 equals the host encoding: %s;  total bytes equal: %s" %
      (min(host_s) * 1e3 / enc[0], enc[0] / conv[0], same0, same_total))
assert same0 and same_total
assert not effort or (r[:, 0] <= per_file0).all(), "a file came out longer than at the base effort"
