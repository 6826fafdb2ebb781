"""Not a test: the FLAC subset of include/dsd2dxd_amd.h ("FLAC frames on the GPU") restated in plain Python from the format
description, the subset decoder of test_host_driver.py with its CRC checks, and the signals both FLAC test files use.

A frame: sync 0xFFF8; block-size code 0xC (4096) or 0x7 (16-bit n - 1 at the header's end); sample-rate code 0; channels - 1;
sample-size code 4 / 5 / 6 and a zero bit; the frame number in the "UTF-8" form; CRC-8 (x^8 + x^2 + x + 1) of the header.  Then one
subframe per channel, bit after bit: fixed order 2 (`0 001010 0`, two warm-up samples, `01 0000 kkkkk`, one Rice code per
residual) for n > 2, verbatim (`0 000001 0`, the samples) otherwise.  Zero bits to the next byte, CRC-16 (x^16 + x^15 + x^2 + 1,
init 0) of everything before it, big-endian."""
import numpy as np

BLOCK = 4096
SIZE_CODE = {16: 4, 20: 5, 24: 6}
HEADER_MAX = 13      # 4 fixed bytes, 6 of frame number, 2 of block size, CRC-8


def _crc_table(poly, width):
    top, mask, tab = 1 << (width - 1), (1 << width) - 1, []
    for i in range(256):
        c = i << (width - 8)
        for _ in range(8):
            c = ((c << 1) ^ poly) & mask if c & top else (c << 1) & mask
        tab.append(c)
    return tab


_T8, _T16 = _crc_table(0x07, 8), _crc_table(0x8005, 16)


def crc8(data):
    c = 0
    for b in data:
        c = _T8[c ^ b]
    return c


def crc16(data):
    c = 0
    for b in data:
        c = ((c << 8) & 0xFFFF) ^ _T16[(c >> 8) ^ b]
    return c


def utf8_number(v):
    """the frame number as FLAC codes it: UTF-8's scheme carried on to 36 bits (here: below 2^31, at most 6 bytes)"""
    if v < 0x80:
        return bytes([v])
    n = 1
    while v >= 1 << (5 * n + 6):          # n continuation bytes hold 6 n bits, the lead byte 6 - n more
        n += 1
    lead = (0xFF << (7 - n)) & 0xFF
    return bytes([lead | (v >> (6 * n))] + [0x80 | ((v >> (6 * i)) & 0x3F) for i in range(n - 1, -1, -1)])


def _bits(value, width):
    return np.array([(value >> i) & 1 for i in range(width - 1, -1, -1)], dtype=np.uint8)


def rice_parameter(abs_sum, count):
    mean, k = abs_sum // count, 0
    while k < 30 and (1 << k) < mean:
        k += 1
    return k


def _subframe_bits(s, depth):
    n, mask = len(s), (1 << depth) - 1
    if n <= 2:
        return np.concatenate([_bits(0b00000010, 8)] + [_bits(int(v) & mask, depth) for v in s])
    r = s[2:] - 2 * s[1:-1] + s[:-2]
    k = rice_parameter(int(np.abs(r).sum()), n - 2)
    u = np.where(r >= 0, 2 * r, -2 * r - 1)
    q = u >> k
    ends = np.cumsum(q + 1 + k)
    stop = ends - 1 - k                                       # the one bit that ends each unary run
    body = np.zeros(int(ends[-1]), dtype=np.uint8)
    body[stop] = 1
    if k:
        shifts = np.arange(k - 1, -1, -1)
        body[(stop[:, None] + 1 + np.arange(k)[None, :]).ravel()] = ((u[:, None] >> shifts[None, :]) & 1).astype(np.uint8).ravel()
    return np.concatenate([_bits(0b00010100, 8), _bits(int(s[0]) & mask, depth), _bits(int(s[1]) & mask, depth),
                           _bits(0b01, 2), _bits(0, 4), _bits(k, 5), body])


def encode_frame(block, depth, number):
    """block: int64 array (n, channels), 1 <= n <= 4096"""
    n, ch = block.shape
    hdr = bytearray([0xFF, 0xF8, 0xC0 if n == BLOCK else 0x70, ((ch - 1) << 4) | (SIZE_CODE[depth] << 1)])
    hdr += utf8_number(number)
    if n != BLOCK:
        hdr += (n - 1).to_bytes(2, "big")
    hdr.append(crc8(hdr))
    bits = np.concatenate([_subframe_bits(block[:, c].astype(np.int64), depth) for c in range(ch)])
    data = bytes(hdr) + np.packbits(bits).tobytes()           # packbits pads the last byte with zero bits
    return data + crc16(data).to_bytes(2, "big")


def encode(samples, depth, first_block=0, final=True):
    """samples: int array (frames, channels).  Returns (frame bytes, [frame sizes], frames consumed)."""
    samples = np.asarray(samples, dtype=np.int64)
    frames = samples.shape[0]
    out, sizes = [], []
    nblocks = frames // BLOCK + (1 if final and frames % BLOCK else 0)
    for b in range(nblocks):
        f = encode_frame(samples[b * BLOCK:(b + 1) * BLOCK], depth, first_block + b)
        out.append(f)
        sizes.append(len(f))
    return b"".join(out), sizes, (frames if final else frames // BLOCK * BLOCK)


def frame_bound(channels, depth, n):
    """the closed form of include/dsd2dxd_amd.h: D2D_FLAC_FRAME_BOUND(n)"""
    return 15 + (channels * (19 + 2 * depth + 30 * max(n - 2, 0)) + 7) // 8


def bound_bytes(channels, depth, frames, final):
    rem = frames % BLOCK
    return frames // BLOCK * frame_bound(channels, depth, BLOCK) + (frame_bound(channels, depth, rem) if final and rem else 0)


def decode(data, channels, depth, first_block=0):
    """Decoder for the subset: fixed order 0 / 2 or verbatim, one Rice partition.  Checks sync, the header fields, consecutive frame
    numbers from `first_block`, every CRC-8 and CRC-16.  Returns (int64 array (frames, channels), [frame sizes])."""
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

    out, sizes, number = [], [], first_block
    while pos < len(bits):
        f0 = pos // 8
        assert pos % 8 == 0 and rd(16) == 0xFFF8, "sync"
        bsc = rd(4)
        assert rd(4) == 0 and rd(4) == channels - 1 and rd(3) == SIZE_CODE[depth] and rd(1) == 0
        first = rd(8)
        if first < 0x80:
            num = first
        else:
            n = 1 if first < 0xE0 else 2 if first < 0xF0 else 3 if first < 0xF8 else 4 if first < 0xFC else 5
            num = first & (0x3F >> n)
            for _ in range(n):
                c = rd(8)
                assert c >> 6 == 2
                num = (num << 6) | (c & 0x3F)
        assert num == number, (num, number)
        number += 1
        assert bsc in (0xC, 0x7)
        n = BLOCK if bsc == 0xC else rd(16) + 1
        rd(8)
        hdr_end = pos // 8 - 1
        assert raw[hdr_end] == crc8(raw[f0:hdr_end]), "frame header CRC-8"
        chans = []
        for _ in range(channels):
            assert rd(1) == 0
            t = rd(6)
            assert rd(1) == 0
            if t == 1:
                s = [sgn(rd(depth), depth) for _ in range(n)]
            else:
                order = t - 8
                assert order in (0, 2)
                s = [sgn(rd(depth), depth) for _ in range(order)]
                assert rd(2) == 1 and rd(4) == 0
                k = rd(5)
                for i in range(order, n):
                    stop = bits.index("1", pos)
                    q = stop - pos
                    pos = stop + 1
                    u = (q << k) | rd(k)
                    r = (u >> 1) if not (u & 1) else -((u + 1) >> 1)
                    s.append(r + (2 * s[i - 1] - s[i - 2] if order == 2 else 0))
            chans.append(s)
        pad = -pos % 8
        assert rd(pad) == 0, "padding bits"
        assert rd(16) == crc16(raw[f0:pos // 8 - 2]), "frame CRC-16"
        sizes.append(pos // 8 - f0)
        out.extend(zip(*chans))
    return np.array(out, dtype=np.int64).reshape(-1, channels), sizes


# ---- signals and PCM packing ---------------------------------------------------------------------------------------------------

SIGNALS = ("silence", "alternate", "spike", "random", "sine")


def signal(name, frames, channels, depth, seed=0):
    """int64 (frames, channels): digital silence (k = 0, one bit per residual); alternating +/- full scale (largest residuals, largest
    k); one full-scale spike in silence (unary runs of thousands of zero bits); uniform random; a full-scale 1 kHz sine at 88.2 kHz"""
    hi, lo = (1 << (depth - 1)) - 1, -(1 << (depth - 1))
    i = np.arange(frames, dtype=np.int64)[:, None]
    c = np.arange(channels, dtype=np.int64)[None, :]
    if name == "silence":
        return np.zeros((frames, channels), dtype=np.int64)
    if name == "alternate":
        return np.where((i + c) % 2 == 0, hi, lo).astype(np.int64)
    if name == "spike":
        s = np.zeros((frames, channels), dtype=np.int64)
        for ch in range(channels):
            if frames:
                s[(frames // 2 + 37 * ch) % frames, ch] = hi if ch % 2 == 0 else lo
        return s
    if name == "random":
        return np.random.default_rng(seed).integers(lo, hi + 1, size=(frames, channels), dtype=np.int64)
    if name == "sine":
        return np.rint(hi * np.sin(2 * np.pi * 1000.0 * i / 88200.0 + 0.7 * c)).astype(np.int64)
    raise ValueError(name)


def _clip(s, depth):
    return np.clip(s, -(1 << (depth - 1)), (1 << (depth - 1)) - 1).astype(np.int64)


def noise(frames, channels, depth, amp_bits, seed):
    """int64 (frames, channels): uniform noise in +/- 2^amp_bits, clipped to the depth.  amp_bits may be fractional (the amplitude is
    rounded): the Rice parameter follows the amplitude, and whole steps alone leave some values of k out."""
    amp = int(round(2.0 ** amp_bits))
    return _clip(np.random.default_rng(seed).integers(-amp, amp + 1, size=(frames, channels), dtype=np.int64), depth)


def residuals(s):
    """the order-2 residuals of one channel (n > 2): r[i] = s[i] - 2 s[i-1] + s[i-2] for i = 2 .. n-1"""
    s = np.asarray(s, dtype=np.int64)
    return s[2:] - 2 * s[1:-1] + s[:-2]


def rice_stats(s):
    """(k, the longest unary run in bits) of one channel of one block, as every encoder here must choose and write them"""
    if len(s) <= 2:
        return None, 0
    r = residuals(s)
    k = rice_parameter(int(np.abs(r).sum()), len(r))
    u = np.where(r >= 0, 2 * r, -2 * r - 1)
    return k, int((u >> k).max())


def tuned_sum(depth, n, target, seed):
    """int64 (n,): one channel whose n - 2 order-2 residuals have sum |r| == target exactly: the mean that decides k sits where the
    caller puts it.  Noise is scaled (by bisection) until the sum over all residuals but the last is just below the target; the last
    sample, which r[n-1] alone depends on, makes up the difference."""
    assert n >= 4 and target >= 0
    u = np.random.default_rng(seed).uniform(-1.0, 1.0, n - 1)
    top = float(1 << (depth - 3))                              # |s| <= 2^(depth-3): the last sample stays within the depth below

    def part(a):
        s = np.rint(u * a).astype(np.int64)
        return s, int(np.abs(residuals(s)).sum())

    assert part(top)[1] > target, "the target is beyond what noise of this depth reaches"
    lo, hi = 0.0, top                                          # part(lo) <= target < part(hi)
    for _ in range(80):
        mid = 0.5 * (lo + hi)
        if part(mid)[1] > target:
            hi = mid
        else:
            lo = mid
    s, p = part(lo)
    d = target - p
    assert 0 <= d <= 1 << (depth - 3), (d, target)
    base = 2 * int(s[-1]) - int(s[-2])                         # the last sample that would make r[n-1] zero
    last = base - d if base > 0 else base + d                  # |r[n-1]| = d, stepping towards zero
    out = np.concatenate([s, [last]]).astype(np.int64)
    assert -(1 << (depth - 1)) <= last < (1 << (depth - 1))
    assert int(np.abs(residuals(out)).sum()) == target
    return out


def spike_at(frames, channels, depth, index, amp, floor_amp):
    """int64 (frames, channels): silence (floor_amp = 0) or uniform +/- floor_amp noise, and one sample of height amp at `index` of
    every channel: +amp in the even channels, -amp in the odd ones"""
    if floor_amp:
        s = np.random.default_rng(1000 * index + frames).integers(-floor_amp, floor_amp + 1, size=(frames, channels), dtype=np.int64)
    else:
        s = np.zeros((frames, channels), dtype=np.int64)
    for c in range(channels):
        s[index, c] = amp if c % 2 == 0 else -amp
    return _clip(s, depth)


def varying(frames, channels, depth, seed):
    """int64 (frames, channels): noise whose amplitude is drawn anew for every block of 4096 (2^0 .. 2^(depth-2)), so that the frames
    of one file differ in size by orders of magnitude"""
    rng = np.random.default_rng(seed)
    u = rng.uniform(-1.0, 1.0, size=(frames, channels))
    bits = rng.integers(0, depth - 1, size=frames // BLOCK + 1)
    amp = (1 << bits[np.arange(frames) // BLOCK]).astype(np.float64)
    return _clip(np.rint(u * amp[:, None]), depth)


def pack_pcm(samples, depth, seed=0):
    """interleaved little-endian frames as the translate calls write them: 16-bit in 2 bytes, 24-bit in 3, 20-bit in the upper 20 bits
    of a 3-byte container (the low nibble is filled with noise here: the encoders must shift it away)"""
    s = np.asarray(samples, dtype=np.int64)
    if depth == 16:
        return s.astype("<i2").view(np.uint8).reshape(-1).copy()
    v = s if depth == 24 else (s << 4) | np.random.default_rng(seed + 99).integers(0, 16, size=s.shape, dtype=np.int64)
    return (v & 0xFFFFFF).astype("<u4").view(np.uint8).reshape(-1, 4)[:, :3].reshape(-1).copy()


def unpack_pcm(pcm, channels, depth):
    b = np.frombuffer(bytes(pcm), dtype=np.uint8) if not isinstance(pcm, np.ndarray) else pcm.view(np.uint8).reshape(-1)
    if depth == 16:
        return b.view("<i2").astype(np.int64).reshape(-1, channels)
    t = b.reshape(-1, 3).astype(np.int64)
    v = t[:, 0] | (t[:, 1] << 8) | (t[:, 2] << 16)
    v = np.where(v & 0x800000, v - (1 << 24), v)
    return (v >> 4 if depth == 20 else v).reshape(-1, channels)
