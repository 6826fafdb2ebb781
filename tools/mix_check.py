"""Measures what profiles/mix_check.md reports, in one GPU session, at the bench workload's sizes: N files of T seconds, six channels,
DSD64 -> 88.2 kHz, 24-bit TPDF, planar 4096, every file's bits distinct (drawn on the device: the kernels' time does not depend on them).

  1. the step of the engine mixed with the 5.1 preset (FIR into the scratch, the mix pass, the history kernel);
  2. the same engine unmixed (the fp6 kernel stores whole six-channel frames, no scratch);
  3. the 'N'-dither step of the same shape: the existing two-pass route (the same FIR pass into the scratch, then the noise shaper);
  4. the mix pass alone: the mixed engine's step bracket minus its FIR bracket (d2d_profile_read_all), minus the history kernel, which is
     what the UNMIXED engine's step bracket holds besides its FIR bracket (the same kernel on the same streams; reported too);
  5. a device-to-device copy that moves the bytes the mix pass moves: it reads 4 bytes per input sample and writes 3 per output
     sample, so a copy of half that sum reads and writes as much.

The five alternate, round after round, after a warm-up of all.  usage: python tools/mix_check.py [--files 64] [--seconds 60] [--rounds 5]
[--steps 3] [--out profiles/mix_check.md]

The kernel's register, LDS and scratch use is the compiler's own report for gfx950 (hipcc -Rpass-analysis=kernel-resource-usage on
mix/d2d_mix.hip), appended where hipcc is found."""
import argparse
import os
import re
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KW = dict(dsd_rate=1, output_rate=88200, channels=6, fmt="P", endianness="L", block_size=4096, filter="E", bit_depth=24, dither="T", seed=206)


def kernel_resources():
    """one line per instantiation of d2d_mix_kernel: VGPRs, SGPRs, static LDS, scratch, occupancy"""
    hipcc = "/opt/rocm/bin/hipcc"
    src = os.path.join(ROOT, "dsd2dxd_amd", "csrc", "mix", "d2d_mix.hip")
    if not os.path.exists(hipcc):
        return ["(hipcc not found)"]
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-Rpass-analysis=kernel-resource-usage",
                        "-c", src, "-o", os.devnull], capture_output=True, text=True, cwd=os.path.dirname(src))
    out, cur = [], None
    for ln in r.stderr.splitlines():
        m = re.search(r"Function Name: \S*d2d_mix_kernelILi(\d+)ELi(\d+)E", ln)
        if m:
            cur = {"name": f"d2d_mix_kernel<{m.group(1)}, {m.group(2)}>"}
            out.append(cur)
            continue
        m = re.search(r"remark:\s+(VGPRs|TotalSGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)", ln)
        if m and cur is not None:
            cur[m.group(1)] = m.group(2)
    return [f"- {k['name']}: {k.get('VGPRs')} VGPRs, {k.get('TotalSGPRs')} SGPRs, {k.get('LDS Size [bytes/block]')} B of static LDS (the matrix and the frame "
            f"image are dynamic: rows x channels x 4 + 256 K x rows x sample bytes), {k.get('ScratchSize [bytes/lane]')} B of scratch per lane, "
            f"{k.get('Occupancy [waves/SIMD]')} waves per SIMD" for k in out] or ["(no report)"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=60.0)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mix_check.md"))
    args = ap.parse_args()
    import torch
    import dsd2dxd_amd as d
    assert torch.cuda.is_available(), "mix_check needs a GPU"
    n, C_ = args.files, 6
    bpc = max(1, int(round(args.seconds * 2822400 / 8 / 4096))) * 4096
    g = torch.Generator(device="cuda").manual_seed(7)
    d_in = [torch.randint(0, 256, (bpc * C_,), dtype=torch.uint8, device="cuda", generator=g) for _ in range(n)]
    engines = {"mixed 5.1 -> stereo": d.Engine(n_files=n, mix=d.mix_preset(6, 2), **KW), "unmixed": d.Engine(n_files=n, **KW),
               "dither N": d.Engine(n_files=n, **dict(KW, dither="N"))}
    frames = engines["unmixed"].next_frames(bpc)
    d_out = torch.empty((n, (frames * 18 + 31) // 16 * 16), dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    ios = {}
    for name, e in engines.items():
        io = (d.FileIO * n)()
        for f in range(n):
            io[f].dsd, io[f].bytes_per_channel, io[f].pcm, io[f].pcm_capacity_bytes = d_in[f].data_ptr(), bpc, d_out[f].data_ptr(), frames * e.frame_bytes
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

    moved = n * frames * (4 * C_ + 3 * 2)                               # bytes the mix pass reads and writes
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
    res = {k: [] for k in list(engines) + ["mix pass alone", "FIR into the scratch", "history kernel", "d2d copy"]}
    for _ in range(args.rounds):
        rest = {}
        for name in engines:
            st, fir = step(name)
            res[name].append(st)
            rest[name] = st - fir
            if name.startswith("mixed"):
                res["FIR into the scratch"].append(fir)
        res["history kernel"].append(rest["unmixed"])
        res["mix pass alone"].append(rest["mixed 5.1 -> stereo"] - rest["unmixed"])
        res["d2d copy"].append(copy())
    lines = [f"{n} files x {args.seconds:g} s, 6 channels, DSD64 -> 88.2 kHz, 24-bit TPDF; {frames} frames per file; {args.rounds} rounds of {args.steps} calls, ms per call",
             "", "| what | median ms | min | max |", "|---|---|---|---|"]
    for k, v in res.items():
        lines.append(f"| {k} | {statistics.median(v):.3f} | {min(v):.3f} | {max(v):.3f} |")
    mp, cp = statistics.median(res["mix pass alone"]), statistics.median(res["d2d copy"])
    lines += ["", f"the mix pass moves {moved / 1e9:.3f} GB per call: {moved / mp / 1e6:.0f} GB/s; the copy of the same bytes: {moved / cp / 1e6:.0f} GB/s; "
                  f"pass / copy = {mp / cp:.2f}",
              f"kernels: mixed {engines['mixed 5.1 -> stereo'].kernel_name()}; unmixed {engines['unmixed'].kernel_name()}; N {engines['dither N'].kernel_name()}"]
    lines += ["", "kernel resources (gfx950, the compiler's report):"] + kernel_resources()
    text = "\n".join(lines)
    print(text, flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    for e in engines.values():
        e.close()


if __name__ == "__main__":
    main()
