#!/usr/bin/env python3
"""One line per kernel of some `hipcc --cuda-device-only -S` listings: tools/isa_digest.py a.s b.s ... > digest.txt

The line is the kernel's symbol, the sha256 of its instructions, `mn=` the sha256 of its sorted instruction mnemonics and its metadata
(registers, spills, scratch, LDS, kernarg bytes).  Two trees whose digests `diff` empty ship the same device code: what a refactor of
host code, file layout or the build has to show.  A refactor of device code that only makes the compiler order or number things
differently changes the first hash and leaves the second and the metadata alone: the same instructions in another order or in other
registers (compare with `cut -d" " -f1,3-`).  Comments are dropped and the numbers of local labels (.LBB<n>_: the kernel's position in
its file) normalised, as in tools/isa_blocks.py."""
import hashlib, re, sys

META = (".vgpr_count", ".agpr_count", ".sgpr_count", ".vgpr_spill_count", ".sgpr_spill_count", ".private_segment_fixed_size",
        ".group_segment_fixed_size", ".kernarg_segment_size", ".max_flat_workgroup_size")


def kernels(path):
    lines = open(path).read().split("\n")
    # metadata: the entries of amdhsa.kernels (keys at four columns; the arguments' own keys sit deeper)
    meta, cur = {}, None
    for l in lines[next((i for i, l in enumerate(lines) if l.startswith("amdhsa.kernels:")), len(lines)):]:
        if l.startswith("  - ."): cur = {}
        if cur is not None and re.match(r"^  [ -] \.\w+:", l):
            k, v = l[4:].split(":", 1)
            cur[k] = v.strip()
            if k == ".name": meta[cur[".name"]] = cur
        if l.startswith("amdhsa.target"): break
    out = {}
    for name in meta:
        start = next(i for i, l in enumerate(lines) if l.startswith(name + ":"))
        h, mn = hashlib.sha256(), []
        for l in lines[start + 1:]:
            if l.startswith(".Lfunc_end") or ".amdhsa_kernel" in l: break
            t = re.sub(r"\.L([A-Za-z_]+)\d+_", r".L\1_", l.split(";")[0]).strip()
            if t and not t.startswith(".section") and not t.startswith(".p2align"):
                h.update((" ".join(t.split()) + "\n").encode())
                if not t.startswith(".") and not t.endswith(":"): mn.append(t.split()[0])
        out[name] = h.hexdigest() + " mn=" + hashlib.sha256("\n".join(sorted(mn)).encode()).hexdigest() + " " + " ".join("%s=%s" % (k[1:], meta[name].get(k, "-")) for k in META)
    return out


if __name__ == "__main__":
    allk = {}
    for p in sys.argv[1:]:
        for name, d in kernels(p).items():
            if allk.setdefault(name, d) != d: sys.exit("%s: %s differs from an earlier listing's" % (p, name))
    for name in sorted(allk): print(name, allk[name])
    print("# %d kernels" % len(allk), file=sys.stderr)
