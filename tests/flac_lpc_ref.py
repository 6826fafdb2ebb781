"""Not a test: FLAC effort 12 (rules 9 to 19 at the head of dsd2dxd_amd/csrc/flac/flac_frame_enc.h) restated in plain Python, and a
decoder of its own for what it writes, written from the FLAC format description: it reads verbatim, fixed and LPC subframes, checks
both CRCs with its own bitwise CRC code and shares nothing with the encoder.

The integer parts (window, autocorrelation, residuals) are exact in numpy's int64; rule 13, the way from the autocorrelation to the
quantised coefficients, is Python ints and Python floats: IEEE doubles, one operation per operation written, never contracted.

For a frame of n samples per channel and each candidate signal x of b bits (flac_search_ref, rule 2):
   9. n < 64: the effort-1 frame.
  10. (o1, p1, cost1) = flac_search_ref.plan(x, b).
  11. w(i) = (i + 1)(n - i); s = bit length of floor((n + 1) / 2) floor((n + 2) / 2); y(i) = (x(i) w(i)) >> s.
  12. R(l) = sum over i = l .. n-1 of y(i) y(i - l), l = 0 .. 12.
  13. R(0) == 0: no candidates.  Levinson-Durbin in f64 as written in the header; it stops for good the first time !(err > 0), and
      that m is not reached.  For m in {4, 8, 12} reached: every |a[j]| < 2^13 and cmax = max |a[j]| > 0, else no candidate; e the
      smallest integer with cmax < 2^e; sh = min(15, 13 - e); error feedback t = 0: t = t + a[j] 2^sh, q[j] = clamp(floor(t + 0.5),
      -8192, 8191), t = t - q[j]; dropped when sum |q[j]| > 62 * 2^sh.
  14. r(i) = x(i) - ((sum over j = 1 .. P of q[j] x(i - j)) >> sh), i >= P.
  15. cost_lpc(P, p) = 8 + P b + 4 + 5 + 14 P + 2 + 4 + the partition terms with o = P.
  16. The P with the least cost_lpc(P, 0), the smaller at a tie; its partition order as at effort 1: cost2.
  17. LPC only if cost2 < cost1.
  18. Stereo as at effort 1, on the final costs.
  19. Subframe: 0, 1ppppp (P - 1), 0; P warm-up samples; 1101; sh in 5 bits; P coefficients of 14 bits; 01, pppp, the partitions."""
import math

import numpy as np

import flac_ref
import flac_search_ref as S

BLOCK = flac_ref.BLOCK
ORDERS = (4, 8, 12)
MIN_FRAME = 64


def window_shift(n):
    return (((n + 1) // 2) * ((n + 2) // 2)).bit_length()


def autocorrelation(x):
    """x: int64 array -> [R(0) .. R(12)] as Python ints"""
    n = len(x)
    i = np.arange(n, dtype=np.int64)
    y = (x * ((i + 1) * (n - i))) >> window_shift(n)
    return [int(np.dot(y[l:], y[:n - l])) for l in range(13)]


def quantise(a, m):
    """a[1 .. m] -> (q[1 .. m] as a list, sh), or None"""
    mags = [abs(v) for v in a[1:m + 1]]
    if any(not (v < 8192.0) for v in mags):
        return None
    cmax = max(mags)
    if cmax == 0.0:
        return None
    e = -1100
    while not cmax < math.ldexp(1.0, e):
        e += 1
    sh = min(15, 13 - e)
    t, q = 0.0, []
    for j in range(1, m + 1):
        t = t + a[j] * float(1 << sh)
        v = max(-8192, min(8191, math.floor(t + 0.5)))
        q.append(v)
        t = t - float(v)
    if sum(abs(v) for v in q) > 62 << sh:
        return None
    return q, sh


def coefficients(R):
    """rule 13: {P: (q, sh)} for the candidates that exist, and how the recursion ended: ("silence" | "stopped", m | "full"), and
    the orders whose candidate was dropped"""
    out, dropped = {}, []
    if R[0] == 0:
        return out, "silence", dropped
    a = [0.0] * 13
    err = float(R[0])
    for m in range(1, 13):
        acc = float(R[m])
        for j in range(1, m):
            acc = acc - a[j] * float(R[m - j])
        k = acc / err
        new = list(a)
        for j in range(1, m):
            new[j] = a[j] - k * a[m - j]
        new[m] = k
        a = new
        err = err * (1.0 - k * k)
        if not err > 0:
            return out, ("stopped", m), dropped
        if m in ORDERS:
            c = quantise(a, m)
            if c is None:
                dropped.append(m)
            else:
                out[m] = c
    return out, "full", dropped


def residuals(x, q, sh):
    """x: int64 array; -> the residuals for i = P .. n-1"""
    P, n = len(q), len(x)
    pred = np.zeros(n - P, dtype=np.int64)
    for j in range(1, P + 1):
        pred += q[j - 1] * x[P - j:n - j]
    return x[P:] - (pred >> sh)


def _lpc_cost(r, n, P, p, b):
    c, ks = S._cost(r, n, P, p, b)                 # 8 + P b + 2 + 4 + the partition terms
    return c + 4 + 5 + 14 * P, ks


def plan(x, b):
    """The effort-12 search for one signal: flac_search_ref's dict, with lpc (None or (q, sh)) and what it chose from."""
    n = len(x)
    pl = S.plan(x, b)
    pl.update(lpc=None, lpc_costs={}, lpc_part_costs=None, cost1=pl["cost"], cost2=None, sh=None)
    cands, ended, dropped = coefficients(autocorrelation(x))
    pl.update(ended=ended, dropped=dropped)
    if not cands:
        return pl
    res = {P: residuals(x, q, sh) for P, (q, sh) in cands.items()}
    assert all(int(np.abs(r).max(initial=0)) < 1 << 30 for r in res.values())
    pl["lpc_costs"] = {P: _lpc_cost(res[P], n, P, 0, b)[0] for P in sorted(cands)}
    P = min(pl["lpc_costs"], key=lambda o: (pl["lpc_costs"][o], o))
    part = [_lpc_cost(res[P], n, P, p, b) for p in range(S.pmax(n) + 1)]
    costs = [c for c, _ in part]
    p = costs.index(min(costs))
    pl.update(lpc_part_costs=costs, cost2=costs[p], lpc_order=P, sh=cands[P][1])
    if costs[p] < pl["cost"]:
        pl.update(lpc=cands[P], order=P, porder=p, cost=costs[p], ks=part[p][1], r=res[P])
    return pl


def _subframe_bits(pl, n):
    if pl["lpc"] is None:
        return S._subframe_bits(pl, n)
    (q, sh), P, p, b = pl["lpc"], pl["order"], pl["porder"], pl["bits"]
    mask = (1 << b) - 1
    out = [flac_ref._bits((0x20 | (P - 1)) << 1, 8)] + [flac_ref._bits(int(v) & mask, b) for v in pl["x"][:P]]
    out += [flac_ref._bits(0b1101, 4), flac_ref._bits(sh, 5)] + [flac_ref._bits(v & 0x3FFF, 14) for v in q]
    out += [flac_ref._bits(0b01, 2), flac_ref._bits(p, 4)]
    for (lo, hi), k in zip(S._partitions(n, P, p), pl["ks"]):
        out += [flac_ref._bits(k, 5), S._rice_bits(S._zigzag(pl["r"][lo - P:hi - P]), k)]
    return np.concatenate(out)


def encode_frame(block, depth, number):
    """block: int64 (n, channels).  Returns (frame bytes, info): info["plans"] lists the plans of ALL candidate signals (what the
    decisions are counted from), info["subs"] those written, info["mode"] the assignment; None / empty below 64 samples."""
    n, ch = block.shape
    if n < MIN_FRAME:
        return S.encode_frame(block, depth, number)[0], dict(mode=None, plans=[], subs=[], totals=None)
    x = [block[:, c].astype(np.int64) for c in range(ch)]
    mode, totals = "independent", None
    if ch == 2:
        L, R = plan(x[0], depth), plan(x[1], depth)
        M, Sd = plan((x[0] + x[1]) >> 1, depth), plan(x[0] - x[1], depth + 1)
        totals = [L["cost"] + R["cost"], L["cost"] + Sd["cost"], Sd["cost"] + R["cost"], M["cost"] + Sd["cost"]]
        mode = S.MODES[totals.index(min(totals))]
        subs = {"independent": [L, R], "left/side": [L, Sd], "side/right": [Sd, R], "mid/side": [M, Sd]}[mode]
        plans = [L, R, M, Sd]
    else:
        subs = plans = [plan(v, depth) for v in x]
    hdr = bytearray([0xFF, 0xF8, 0xC0 if n == BLOCK else 0x70, (S.MODE_NIBBLE.get(mode, ch - 1) << 4) | (flac_ref.SIZE_CODE[depth] << 1)])
    hdr += flac_ref.utf8_number(number)
    if n != BLOCK:
        hdr += (n - 1).to_bytes(2, "big")
    hdr.append(flac_ref.crc8(hdr))
    data = bytes(hdr) + np.packbits(np.concatenate([_subframe_bits(pl, n) for pl in subs])).tobytes()
    return data + flac_ref.crc16(data).to_bytes(2, "big"), dict(mode=mode, plans=plans, subs=subs, totals=totals)


def encode(samples, depth, first_block=0, final=True):
    """samples: int array (frames, channels).  Returns (frame bytes, [frame sizes], frames consumed, [info per frame])."""
    samples = np.asarray(samples, dtype=np.int64)
    frames = samples.shape[0]
    out, sizes, infos = [], [], []
    for b in range(frames // BLOCK + (1 if final and frames % BLOCK else 0)):
        f, info = encode_frame(samples[b * BLOCK:(b + 1) * BLOCK], depth, first_block + b)
        out.append(f)
        sizes.append(len(f))
        infos.append(info)
    return b"".join(out), sizes, (frames if final else frames // BLOCK * BLOCK), infos


# ---- the decoder, from the format description: nothing above is used below -----------------------------------------------------------

_FIXED = {0: (), 1: (1,), 2: (2, -1), 3: (3, -3, 1), 4: (4, -6, 4, -1)}
_SIZE = {4: 16, 5: 20, 6: 24}


def _crc(data, poly, width):
    c, top, mask = 0, 1 << (width - 1), (1 << width) - 1
    for byte in data:
        c ^= byte << (width - 8)
        for _ in range(8):
            c = ((c << 1) ^ poly) & mask if c & top else (c << 1) & mask
    return c


def decode(data, channels, depth, first_block=0):
    """Returns (int64 array (frames, channels), [frame sizes], [(assignment nibble, [(kind, order, partition order)])]) with kind
    'verbatim', 'fixed' or 'lpc'.  Asserts sync, the header fields, consecutive frame numbers, every CRC-8 and CRC-16."""
    raw = bytes(data)
    bits = "".join(f"{v:08b}" for v in raw)
    pos = 0

    def rd(k):
        nonlocal pos
        v = int(bits[pos:pos + k], 2) if k else 0
        pos += k
        return v

    def rds(k):
        v = rd(k)
        return v - (1 << k) if v >> (k - 1) else v

    def residual(n, order, s, predict):
        nonlocal pos
        assert rd(2) == 1, "residual coding method"
        porder = rd(4)
        assert n % (1 << porder) == 0 and (n >> porder) >= order
        for j in range(1 << porder):
            k = rd(5)
            assert k != 31, "escape"
            for _ in range((n >> porder) - (order if j == 0 else 0)):
                stop = bits.index("1", pos)
                u = ((stop - pos) << k)
                pos = stop + 1
                u |= rd(k)
                s.append((-(u + 1) >> 1 if u & 1 else u >> 1) + predict(s))
        assert len(s) == n
        return porder

    def subframe(n, bps):
        assert rd(1) == 0
        t = rd(6)
        assert rd(1) == 0, "wasted bits"
        if t == 1:
            return [rds(bps) for _ in range(n)], ("verbatim", 0, 0)
        if 8 <= t <= 12:
            order = t - 8
            s = [rds(bps) for _ in range(order)]
            coef = _FIXED[order]
            return s, ("fixed", order, residual(n, order, s, lambda v: sum(c * v[-1 - m] for m, c in enumerate(coef))))
        assert t >= 32, ("subframe type", t)
        order = t - 31
        s = [rds(bps) for _ in range(order)]
        precision = rd(4) + 1
        assert precision != 16
        shift = rds(5)
        assert shift >= 0
        coef = [rds(precision) for _ in range(order)]
        return s, ("lpc", order, residual(n, order, s, lambda v: sum(c * v[-1 - m] for m, c in enumerate(coef)) >> shift))

    out, sizes, infos, number = [], [], [], first_block
    while pos < len(bits):
        f0 = pos // 8
        assert pos % 8 == 0 and rd(15) == 0x7FFC and rd(1) == 0, "sync, fixed block size"
        bsc, rate, assign, size, zero = rd(4), rd(4), rd(4), rd(3), rd(1)
        assert rate == 0 and zero == 0 and _SIZE[size] == depth
        assert assign == channels - 1 or (channels == 2 and assign in (8, 9, 10)), assign
        first = rd(8)
        num = first
        if first >= 0x80:
            m = 1 if first < 0xE0 else 2 if first < 0xF0 else 3 if first < 0xF8 else 4 if first < 0xFC else 5
            num = first & (0x3F >> m)
            for _ in range(m):
                c = rd(8)
                assert c >> 6 == 2
                num = (num << 6) | (c & 0x3F)
        assert num == number, (num, number)
        number += 1
        assert bsc in (0xC, 0x7)
        n = 4096 if bsc == 0xC else rd(16) + 1
        assert rd(8) == _crc(raw[f0:pos // 8 - 1], 0x07, 8), "frame header CRC-8"
        side = {8: 1, 9: 0, 10: 1}.get(assign)
        subs = [subframe(n, depth + 1 if c == side else depth) for c in range(channels)]
        chans = [np.array(s, dtype=np.int64) for s, _ in subs]
        if assign == 8:
            chans = [chans[0], chans[0] - chans[1]]
        elif assign == 9:
            chans = [chans[0] + chans[1], chans[1]]
        elif assign == 10:
            mid = (chans[0] << 1) | (chans[1] & 1)
            chans = [(mid + chans[1]) >> 1, (mid - chans[1]) >> 1]
        assert rd(-pos % 8) == 0, "padding bits"
        assert rd(16) == _crc(raw[f0:pos // 8 - 2], 0x8005, 16), "frame CRC-16"
        sizes.append(pos // 8 - f0)
        infos.append((assign, [i for _, i in subs]))
        out.append(np.stack(chans, axis=1))
    pcm = np.concatenate(out) if out else np.zeros((0, channels), dtype=np.int64)
    return pcm, sizes, infos
