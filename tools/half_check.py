"""Measures what profiles/half_check.md reports, in one GPU session, on the bench batch: N files of T seconds, stereo, DSD64, 24-bit TPDF,
planar 4096, every file's bits distinct (drawn on the device: the kernels' time does not depend on them).

  1. the step of the halved engine, 44.1 kHz (d2d_create_half: the FIR of 88.2 kHz into the scratch, the half pass, the two history kernels);
  2. the 88.2 kHz engine with dither T (the flagship step: the fp6 kernel stores the frames itself) and with dither X (the same without the
     per-call dither table: what its step bracket holds besides its FIR bracket is the history kernel alone);
  3. the 'N'-dither step at 88.2 kHz: the same FIR pass into the scratch, then the noise shaper;
  4. the halved engine's FIR pass (its FIR bracket) and its half pass apart: the step bracket minus the FIR bracket (d2d_profile_read_all)
     minus the history kernel of 2. (the carry of the NT - 1 sums, a block per stream, stays inside the figure);
  5. a device-to-device copy that moves the bytes the half pass moves: it reads 4 bytes per sum and writes 3 per output sample, so a copy of
     half that sum reads and writes as much.

They alternate, round after round, after a warm-up of all.  usage: python tools/half_check.py [--files 64] [--seconds 60] [--rounds 5]
[--steps 3] [--out profiles/half_check.md]

The kernel's register, LDS and scratch use is the compiler's own report for gfx950 (hipcc -Rpass-analysis=kernel-resource-usage on
half/d2d_half.hip), appended where hipcc is found."""
import argparse
import os
import re
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KW = dict(dsd_rate=1, output_rate=88200, channels=2, fmt="P", endianness="L", block_size=4096, filter="E", bit_depth=24, dither="T", seed=206)


def kernel_resources():
    hipcc = "/opt/rocm/bin/hipcc"
    src = os.path.join(ROOT, "dsd2dxd_amd", "csrc", "half", "d2d_half.hip")
    if not os.path.exists(hipcc):
        return ["(hipcc not found)"]
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-Rpass-analysis=kernel-resource-usage",
                        "-c", src, "-o", os.devnull], capture_output=True, text=True, cwd=os.path.dirname(src))
    out, cur = [], None
    for ln in r.stderr.splitlines():
        m = re.search(r"Function Name: \S*?(d2d_half\w*?kernel)E", ln)
        if m:
            cur = {"name": m.group(1)}
            out.append(cur)
            continue
        m = re.search(r"remark:\s+(VGPRs|TotalSGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)", ln)
        if m and cur is not None:
            cur[m.group(1)] = m.group(2)
    return [f"- {k['name']}: {k.get('VGPRs')} VGPRs, {k.get('TotalSGPRs')} SGPRs, {k.get('LDS Size [bytes/block]')} B of static LDS, "
            f"{k.get('ScratchSize [bytes/lane]')} B of scratch per lane, {k.get('Occupancy [waves/SIMD]')} waves per SIMD" for k in out] or ["(no report)"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=60.0)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "half_check.md"))
    args = ap.parse_args()
    import torch
    import dsd2dxd_amd as d
    assert torch.cuda.is_available(), "half_check needs a GPU"
    n, C_ = args.files, 2
    bpc = max(1, int(round(args.seconds * 2822400 / 8 / 4096))) * 4096
    g = torch.Generator(device="cuda").manual_seed(7)
    d_in = [torch.randint(0, 256, (bpc * C_,), dtype=torch.uint8, device="cuda", generator=g) for _ in range(n)]
    HALF, T_, X_, N_ = "halved, 44.1 kHz T", "88.2 kHz T", "88.2 kHz X", "88.2 kHz N"
    engines = {HALF: d.Engine.create_half(n_files=n, **dict(KW, output_rate=44100)), T_: d.Engine(n_files=n, **KW),
               X_: d.Engine(n_files=n, **dict(KW, dither="X")), N_: d.Engine(n_files=n, **dict(KW, dither="N"))}
    sums = engines[T_].next_frames(bpc)
    frames = engines[HALF].next_frames(bpc)
    assert frames == (sums + 1) // 2
    d_out = torch.empty((n, (sums * 6 + 31) // 16 * 16), dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    ios = {}
    for name, e in engines.items():
        io = (d.FileIO * n)()
        for f in range(n):
            io[f].dsd, io[f].bytes_per_channel, io[f].pcm, io[f].pcm_capacity_bytes = d_in[f].data_ptr(), bpc, d_out[f].data_ptr(), e.next_frames(bpc) * e.frame_bytes
        ios[name] = io
        e.profile_enable(True)

    def step(name):
        """(step ms, FIR ms) per call over args.steps calls"""
        e = engines[name]
        for _ in range(args.steps):
            e.translate_batch_device(ios[name], stream)
        torch.cuda.synchronize()
        fir, st, launches = e.profile_read_all()
        return st / launches, fir / launches

    moved = n * C_ * (sums * 4 + frames * 3)                            # bytes the half pass reads and writes
    src = torch.empty(moved // 2, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)

    def copy():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.steps):
            dst.copy_(src)
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / args.steps

    for name in engines:
        step(name)
    copy()
    res = {k: [] for k in list(engines) + ["halved: FIR into the scratch", "halved: half pass (with the carry of the sums)", "history kernel", "d2d copy"]}
    for _ in range(args.rounds):
        rest = {}
        for name in engines:
            st, fir = step(name)
            res[name].append(st)
            rest[name] = st - fir
            if name == HALF:
                res["halved: FIR into the scratch"].append(fir)
        res["history kernel"].append(rest[X_])
        res["halved: half pass (with the carry of the sums)"].append(rest[HALF] - rest[X_])
        res["d2d copy"].append(copy())
    macs = n * C_ * frames * len(d.half_taps()[0])
    lines = [f"{n} files x {args.seconds:g} s, stereo, DSD64, 24-bit; {sums} sums and {frames} frames per file; {args.rounds} rounds of {args.steps} calls, ms per call",
             "", "| what | median ms | min | max |", "|---|---|---|---|"]
    for k, v in res.items():
        lines.append(f"| {k} | {statistics.median(v):.3f} | {min(v):.3f} | {max(v):.3f} |")
    hp, cp = statistics.median(res["halved: half pass (with the carry of the sums)"]), statistics.median(res["d2d copy"])
    ht, tt, nt = (statistics.median(res[k]) for k in (HALF, T_, N_))
    lines += ["", f"the half pass makes {macs / 1e9:.1f} G multiply-adds per call: {macs / hp / 1e9:.2f} T multiply-adds/s; it moves {moved / 1e9:.3f} GB: "
                  f"{moved / hp / 1e6:.0f} GB/s; the copy of the same bytes: {moved / cp / 1e6:.0f} GB/s; pass / copy = {hp / cp:.1f}",
              f"halved step / 88.2 kHz T step = {ht / tt:.1f}; halved step / 88.2 kHz N step = {ht / nt:.1f}; half pass / 88.2 kHz T step = {hp / tt:.1f}",
              "kernels: " + "; ".join(f"{k}: {e.kernel_name()}" for k, e in engines.items())]
    lines += ["", "kernel resources (gfx950, the compiler's report; the planes and the frame image are dynamic LDS: 2 x (tile + 196) x 4 + tile x frame bytes,"
              " tile = 1024 frames for frames of at most 64 bytes):"] + kernel_resources()
    text = "\n".join(lines)
    print(text, flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    for e in engines.values():
        e.close()


if __name__ == "__main__":
    main()
