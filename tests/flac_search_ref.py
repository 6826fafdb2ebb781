"""Not a test: FLAC effort 1 (the search that dsd2dxd_amd/csrc/flac/flac_frame_enc.h defines) restated in plain Python, and a
decoder for what it writes, written from the FLAC format description and not from the encoder.

The encoder, for a frame of n samples per channel, ch channels and depth d (header, CRCs and padding as in flac_ref):
  1. n < 16: the effort-0 frame (flac_ref.encode_frame).
  2. Candidate signals: each channel at b = d bits; for ch == 2 also M = (L + R) >> 1 (floor) at b = d and S = L - R at b = d + 1.
  3. Residuals r_0 = x, r_o(i) = r_{o-1}(i) - r_{o-1}(i-1) for i >= o, o = 0 .. 4.
  4. cost(o, p) = 8 + o b + 2 + 4 + sum over the 2^p partitions of (5 + sum of ((u >> k) + 1 + k)), u = zigzag(r); partition j holds
     the residuals with i in [j (n >> p), (j + 1)(n >> p)) and i >= o; its k is the smallest with 2^k >= floor(sum |r| / count),
     at most 30.
  5. The o in 0 .. 4 with the least cost(o, 0), the smallest at a tie.
  6. For that o the p in 0 .. pmax with the least cost(o, p), the smallest at a tie; pmax the largest p <= 6 with n % 2^p == 0 and
     (n >> p) >= 16.
  7. ch == 2: the least of L + R (assignment 0001), L + S (1000), S + R (1001), M + S (1010), the earlier at a tie.
  8. Subframe: 0, 001ooo, 0; o warm-up samples of b bits; 01, pppp; per partition kkkkk and its Rice codes.

The decoder reads any frame of that family: fixed orders 0 .. 4 and verbatim, partition orders 0 .. 6 (5-bit parameters, no escape),
assignments 0 .. 7 (independent), 1000 (left/side), 1001 (side/right), 1010 (mid/side) with a side subframe of d + 1 bits."""
import numpy as np

import flac_ref

BLOCK = flac_ref.BLOCK
MODES = ("independent", "left/side", "side/right", "mid/side")
MODE_NIBBLE = {"left/side": 0x8, "side/right": 0x9, "mid/side": 0xA}


def pmax(n):
    p = 0
    while p < 6 and n % (2 << p) == 0 and (n >> (p + 1)) >= 16:
        p += 1
    return p


def _zigzag(r):
    return np.where(r >= 0, 2 * r, -2 * r - 1)


def _partitions(n, o, p):
    """[(lo, hi)] in sample indices: partition j holds i in [max(j psz, o), (j + 1) psz)"""
    psz = n >> p
    return [(max(j * psz, o), (j + 1) * psz) for j in range(1 << p)]


def _cost(r, n, o, p, b):
    """r: the order-o residuals, r[i - o] for i = o .. n-1.  Returns (cost, [k per partition])."""
    cost, ks = 8 + o * b + 2 + 4, []
    for lo, hi in _partitions(n, o, p):
        part = r[lo - o:hi - o]
        k = flac_ref.rice_parameter(int(np.abs(part).sum()), hi - lo)
        cost += 5 + int(((_zigzag(part) >> k) + 1 + k).sum())
        ks.append(k)
    return cost, ks


def plan(x, b):
    """The search for one signal.  Returns a dict: order, porder, cost, ks, r, and the cost lists it chose from."""
    n = len(x)
    rs = [x]
    for _ in range(4):
        rs.append(rs[-1][1:] - rs[-1][:-1])
    order_costs = [_cost(rs[o], n, o, 0, b)[0] for o in range(5)]
    o = order_costs.index(min(order_costs))                    # index(): the first, so the smallest order at a tie
    part = [_cost(rs[o], n, o, p, b) for p in range(pmax(n) + 1)]
    part_costs = [c for c, _ in part]
    p = part_costs.index(min(part_costs))
    return dict(order=o, porder=p, cost=part_costs[p], ks=part[p][1], r=rs[o], x=x, bits=b, order_costs=order_costs, part_costs=part_costs)


def _rice_bits(u, k):
    q = u >> k
    ends = np.cumsum(q + 1 + k)
    stop = ends - 1 - k
    body = np.zeros(int(ends[-1]), dtype=np.uint8)
    body[stop] = 1
    if k:
        shifts = np.arange(k - 1, -1, -1)
        body[(stop[:, None] + 1 + np.arange(k)[None, :]).ravel()] = ((u[:, None] >> shifts[None, :]) & 1).astype(np.uint8).ravel()
    return body


def _subframe_bits(pl, n):
    o, p, b = pl["order"], pl["porder"], pl["bits"]
    mask = (1 << b) - 1
    out = [flac_ref._bits((8 | o) << 1, 8)] + [flac_ref._bits(int(v) & mask, b) for v in pl["x"][:o]]
    out += [flac_ref._bits(0b01, 2), flac_ref._bits(p, 4)]
    for (lo, hi), k in zip(_partitions(n, o, p), pl["ks"]):
        out += [flac_ref._bits(k, 5), _rice_bits(_zigzag(pl["r"][lo - o:hi - o]), k)]
    return np.concatenate(out)


def encode_frame(block, depth, number):
    """block: int64 (n, channels).  Returns (frame bytes, info); info has the assignment, and per subframe the order, the partition
    order and the cost lists they were chosen from, plus the four stereo totals -- None / empty for a frame below 16 samples."""
    n, ch = block.shape
    if n < 16:
        return flac_ref.encode_frame(block, depth, number), dict(mode=None, orders=[], porders=[], order_costs=[], part_costs=[], totals=None)
    x = [block[:, c].astype(np.int64) for c in range(ch)]
    mode, totals = "independent", None
    if ch == 2:
        L, R = plan(x[0], depth), plan(x[1], depth)
        M, S = plan((x[0] + x[1]) >> 1, depth), plan(x[0] - x[1], depth + 1)
        totals = [L["cost"] + R["cost"], L["cost"] + S["cost"], S["cost"] + R["cost"], M["cost"] + S["cost"]]
        mode = MODES[totals.index(min(totals))]
        subs = {"independent": [L, R], "left/side": [L, S], "side/right": [S, R], "mid/side": [M, S]}[mode]
    else:
        subs = [plan(v, depth) for v in x]
    hdr = bytearray([0xFF, 0xF8, 0xC0 if n == BLOCK else 0x70, (MODE_NIBBLE.get(mode, ch - 1) << 4) | (flac_ref.SIZE_CODE[depth] << 1)])
    hdr += flac_ref.utf8_number(number)
    if n != BLOCK:
        hdr += (n - 1).to_bytes(2, "big")
    hdr.append(flac_ref.crc8(hdr))
    data = bytes(hdr) + np.packbits(np.concatenate([_subframe_bits(pl, n) for pl in subs])).tobytes()
    info = dict(mode=mode, orders=[pl["order"] for pl in subs], porders=[pl["porder"] for pl in subs],
                order_costs=[pl["order_costs"] for pl in subs], part_costs=[pl["part_costs"] for pl in subs], totals=totals)
    return data + flac_ref.crc16(data).to_bytes(2, "big"), info


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


# ---- the decoder, from the format description --------------------------------------------------------------------------------------

_PREDICT = {0: (), 1: (1,), 2: (2, -1), 3: (3, -3, 1), 4: (4, -6, 4, -1)}      # the fixed predictors' coefficients of s[i-1], s[i-2] ...


def decode(data, channels, depth, first_block=0):
    """Checks sync, the header fields, consecutive frame numbers from `first_block`, every CRC-8 and CRC-16.
    Returns (int64 array (frames, channels), [frame sizes], [(assignment nibble, [(order or 'verbatim', partition order)])])."""
    raw = bytes(data)
    bits = "".join(f"{x:08b}" for x in raw)
    pos = 0

    def rd(n):
        nonlocal pos
        x = int(bits[pos:pos + n], 2) if n else 0
        pos += n
        return x

    def sgn(x, n):
        return x - (1 << n) if x >> (n - 1) else x

    def subframe(n, bps):
        nonlocal pos
        assert rd(1) == 0, "subframe padding bit"
        t = rd(6)
        assert rd(1) == 0, "wasted bits are not part of the subset"
        if t == 1:
            return [sgn(rd(bps), bps) for _ in range(n)], ("verbatim", 0)
        assert 8 <= t <= 12, ("subframe type", t)
        order = t - 8
        s = [sgn(rd(bps), bps) for _ in range(order)]
        assert rd(2) == 1, "residual coding method"
        porder = rd(4)
        assert porder <= 6 and n % (1 << porder) == 0 and (n >> porder) >= order
        coef = _PREDICT[order]
        for j in range(1 << porder):
            k = rd(5)
            assert k != 31, "escape"
            for _ in range((n >> porder) - (order if j == 0 else 0)):
                stop = bits.index("1", pos)
                q = stop - pos
                pos = stop + 1
                u = (q << k) | rd(k)
                r = (u >> 1) if not (u & 1) else -((u + 1) >> 1)
                s.append(r + sum(c * s[-1 - m] for m, c in enumerate(coef)))
        assert len(s) == n
        return s, (order, porder)

    out, sizes, infos, number = [], [], [], first_block
    while pos < len(bits):
        f0 = pos // 8
        assert pos % 8 == 0 and rd(16) == 0xFFF8, "sync"
        bsc = rd(4)
        assert rd(4) == 0
        assign = rd(4)
        assert assign == channels - 1 or (channels == 2 and assign in (8, 9, 10)), ("channel assignment", assign)
        assert rd(3) == flac_ref.SIZE_CODE[depth] and rd(1) == 0
        first = rd(8)
        if first < 0x80:
            num = first
        else:
            m = 1 if first < 0xE0 else 2 if first < 0xF0 else 3 if first < 0xF8 else 4 if first < 0xFC else 5
            num = first & (0x3F >> m)
            for _ in range(m):
                c = rd(8)
                assert c >> 6 == 2
                num = (num << 6) | (c & 0x3F)
        assert num == number, (num, number)
        number += 1
        assert bsc in (0xC, 0x7)
        n = BLOCK if bsc == 0xC else rd(16) + 1
        rd(8)
        hdr_end = pos // 8 - 1
        assert raw[hdr_end] == flac_ref.crc8(raw[f0:hdr_end]), "frame header CRC-8"
        side = {8: 1, 9: 0, 10: 1}.get(assign)                   # which subframe is the side channel, one bit wider
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
        assert rd(16) == flac_ref.crc16(raw[f0:pos // 8 - 2]), "frame CRC-16"
        sizes.append(pos // 8 - f0)
        infos.append((assign, [i for _, i in subs]))
        out.append(np.stack(chans, axis=1))
    pcm = np.concatenate(out) if out else np.zeros((0, channels), dtype=np.int64)
    return pcm, sizes, infos
