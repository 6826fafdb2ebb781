#!/usr/bin/env python3
"""Encoding widths and wait-state padding per basic block of one kernel in a hipcc -S listing: tools/isa_enc.py file.s <kernel-name-substring> [mfma count]

One line per block (only those with the given number of MFMAs, if given): vector instructions, how many of them have 64-bit encodings (VOP3: the
`_e64` forms and the instructions that exist in no other form; `_sdwa` / `_dpp`; any instruction with a 32-bit literal), `s_nop` (and how many
of them pad the way to an MFMA) and `s_waitcnt`.  The blocks are tools/isa_blocks.py's."""
import re, sys

path, key = sys.argv[1], sys.argv[2]
want = int(sys.argv[3]) if len(sys.argv) > 3 else None
lines = open(path).read().split("\n")
start = next(i for i, l in enumerate(lines) if l.startswith("_Z") and key in l and (l.rstrip().endswith(":") or (": " in l and "; @" in l)))
INLINE = re.compile(r"^(-?\d+|0x[0-9a-f]+|-?\d+\.\d+)$")


def literal(ops):
    for o in ops:
        o = o.strip()
        if not INLINE.match(o): continue
        if o.startswith("0x"): return True                      # (the printer writes inline integers in decimal)
        if "." in o:
            if abs(float(o)) not in (0.5, 1.0, 2.0, 4.0): return True
        elif not -16 <= int(o) <= 64: return True
    return False


def wide(op, ops):
    if op.endswith("_e32"): return literal(ops)
    return True                                                 # _e64, _sdwa, _dpp, and the VOP3-only instructions (no suffix)


blocks, cur = [], ["entry", []]
for l in lines[start + 1:]:
    if l.startswith(".Lfunc_end"): break
    m = re.match(r"^(\.LBB\d+_\d+):", l)
    if m:
        blocks.append(cur); cur = [m.group(1), []]; continue
    t = l.split(";")[0].strip()
    if not t or t.startswith("."): continue
    cur[1].append(t)
blocks.append(cur)
for name, ins in blocks:
    ops = [(t.split()[0], t.split(None, 1)[1].split(",") if " " in t else []) for t in ins]
    mfma = sum(1 for o, _ in ops if o.startswith("v_mfma"))
    if want is not None and mfma != want: continue
    valu = [(o, a) for o, a in ops if o.startswith("v_") and not o.startswith("v_mfma") and not re.match(r"v_(read|write)(first)?lane", o)]
    n64 = sum(1 for o, a in valu if wide(o, a))
    nops = sum(1 for o, _ in ops if o == "s_nop")
    waits = sum(1 for o, _ in ops if o.startswith("s_waitcnt"))
    pad = 0                                                     # s_nop with nothing but LDS or scalar instructions between it and an MFMA
    for i, (o, _) in enumerate(ops):
        if o != "s_nop": continue
        j = i + 1
        while j < len(ops) and (ops[j][0].startswith("ds_") or ops[j][0].startswith("s_")): j += 1
        pad += j < len(ops) and ops[j][0].startswith("v_mfma")
    print("%-12s mfma=%d valu=%d valu64=%d s_nop=%d (in front of an MFMA: %d) s_waitcnt=%d" % (name, mfma, len(valu), n64, nops, pad, waits))
