"""The cases of the segment calls (include/dsd2dxd_amd.h, "A chunk's bookkeeping in one launch"), written once for the host twins
(tests/test_segments_cpu.py) and the device calls (tests/test_gpu_segments.py).  A `Memory` hands out buffers of one kind -- numpy
arrays, device tensors, pinned tensors -- as (pointer, read, write); the checks compare WHOLE arenas with a numpy model, so every byte
outside the declared ranges is held to what it was, under two complementary fills, with 256 guard bytes around every range."""
import numpy as np

GUARD = 256
FILLS = (0x5A, 0xA5)
SHORT = (0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65)          # every src misalignment against every dst misalignment
LONG = (4095, 4097, 70001)                                  # more than one 16 KiB tile for the last; eight pairs each
PAIRS = ((0, 0), (0, 1), (1, 0), (3, 13), (15, 15), (8, 4), (5, 5), (12, 7))
ERR_PARAM, ERR_CAPACITY = -1, -20
GAVE_UP = 0xFFFFFFFFFFFFFFFF


class HostMemory:
    """numpy arrays (the twins)"""

    def alloc(self, nbytes):
        a = np.zeros(nbytes + 16, dtype=np.uint8)
        off = (-a.ctypes.data) % 16
        v = a[off:off + nbytes]
        return Buffer(v.ctypes.data, lambda: v.copy(), lambda x: v.__setitem__(slice(None), x), keep=a)

    def sync(self):
        pass


class Buffer:
    def __init__(self, ptr, read, write, keep=None):
        self.ptr, self.read, self.write, self.keep = ptr, read, write, keep


def move_plan():
    """[(length, src misalignment, dst misalignment)]: 11 * 256 + 3 * 8 segments, far more than one launch takes"""
    plan = [(n, s, d) for n in SHORT for s in range(16) for d in range(16)]
    plan += [(n, s, d) for n in LONG for s, d in PAIRS]
    return plan


def layout(plan, which):
    """offsets of every range in its arena: a slot per segment, 16-byte aligned, GUARD bytes on both sides of the range"""
    offs, at = [], 0
    for n, s, d in plan:
        offs.append(at + GUARD + (s if which == "src" else d))
        at += (GUARD + 15 + n + GUARD + 15) // 16 * 16
    return np.array(offs, dtype=np.int64), at


def check_move(d, move, src_mem, dst_mem, fill):
    """one call over the whole plan; `move(segs)` is the call under test"""
    plan = move_plan()
    s_off, s_size = layout(plan, "src")
    d_off, d_size = layout(plan, "dst")
    rng = np.random.default_rng(fill)
    src_image = rng.integers(0, 256, s_size, dtype=np.uint8)
    dst_image = np.full(d_size, fill, dtype=np.uint8)
    src, dst = src_mem.alloc(s_size), dst_mem.alloc(d_size)
    assert src.ptr % 16 == 0 and dst.ptr % 16 == 0
    src.write(src_image); dst.write(dst_image)
    segs = (d.Segment * len(plan))()
    want = dst_image.copy()
    for i, (n, _, _) in enumerate(plan):
        segs[i].dst, segs[i].src, segs[i].bytes = dst.ptr + int(d_off[i]), src.ptr + int(s_off[i]), n
        want[d_off[i]:d_off[i] + n] = src_image[s_off[i]:s_off[i] + n]
    move(segs)
    dst_mem.sync()
    got = dst.read()
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{bad.size} bytes differ, the first at arena offset {bad[0]} (fill {fill:#x})"
    assert np.array_equal(src.read(), src_image)


def check_move_refusals(d, move, mem):
    """a dst range that overlaps a src or another dst range: D2D_ERR_PARAM and no byte changes; ranges that touch, and src ranges that
    overlap each other, pass"""
    image = np.arange(4096, dtype=np.uint32).astype(np.uint8)
    buf = mem.alloc(4096)

    def call(triples):
        segs = (d.Segment * len(triples))()
        for i, (to, frm, n) in enumerate(triples):
            segs[i].dst, segs[i].src, segs[i].bytes = buf.ptr + to, buf.ptr + frm, n
        move(segs)
        mem.sync()

    overlapping = [
        [(100, 110, 20)],                                   # its own src, dst in front
        [(110, 100, 20)],                                   # its own src, dst behind
        [(100, 1000, 50), (149, 2000, 10)],                 # another dst, by one byte
        [(100, 1000, 50), (2000, 149, 10)],                 # another segment's src, by one byte
        [(2000, 149, 10), (100, 1000, 50)],                 # ... in the other order
        [(100, 1000, 50), (120, 2000, 5)],                  # a dst inside another dst
        [(3000, 3000, 1)],                                  # one byte onto itself
    ]
    for triples in overlapping:
        buf.write(image)
        try:
            call(triples)
        except d.D2DError as ex:
            assert ex.code == ERR_PARAM and "overlap" in ex.message, ex
        else:
            raise AssertionError(f"{triples} was accepted")
        assert np.array_equal(buf.read(), image), triples
    # null pointers
    segs = (d.Segment * 1)()
    segs[0].dst, segs[0].src, segs[0].bytes = buf.ptr, None, 4
    try:
        move(segs)
    except d.D2DError as ex:
        assert ex.code == ERR_PARAM
    else:
        raise AssertionError("a null src was accepted")
    # what passes: touching ranges, shared and overlapping sources, empty segments anywhere (their pointers are not looked at)
    buf.write(image)
    call([(100, 1000, 50), (150, 1000, 50), (200, 1025, 50), (120, 110, 0), (0, 0, 0)])
    want = image.copy()
    want[100:150] = image[1000:1050]; want[150:200] = image[1000:1050]; want[200:250] = image[1025:1075]
    assert np.array_equal(buf.read(), want)


def pack_lengths(case):
    if case == "few":                                        # zero-length segments at the first, a middle and the last place
        return [0, 5, 4097, 0, 70001, 33, 16, 0]
    rng = np.random.default_rng(3)                           # "many": more sources than one launch takes
    n = list(rng.integers(0, 200, 300))
    n[0], n[127], n[128], n[129], n[299] = 0, 0, 17, 0, 0
    return [int(x) for x in n]


def check_pack(d, pack, mem, dst_mem, case, fill, too_long=None, slack=7):
    """`pack(srcs, dst_ptr, capacity, offsets_ptr)` is the call under test; the lengths live in `mem` (the device reads them there).
    too_long: the index of a source whose length is one above its maximum -- then only the table changes, to all-ones"""
    lengths = pack_lengths(case)
    n = len(lengths)
    maxes = [x + (slack if i % 3 else 0) for i, x in enumerate(lengths)]
    actual = list(lengths)
    if too_long is not None:
        actual[too_long] = maxes[too_long] + 1
    rng = np.random.default_rng(n + fill)
    # sources at every misalignment, a gap between them
    s_off, at = [], 0
    for i, m in enumerate(maxes):
        s_off.append(at + 16 + (i * 7) % 16)
        at += (16 + 15 + m + 1 + 16 + 15) // 16 * 16
    src_image = rng.integers(0, 256, at, dtype=np.uint8)
    src = mem.alloc(at); src.write(src_image)
    lens = mem.alloc(8 * n); lens.write(np.array(actual, dtype="<u8").view(np.uint8))
    cap = sum(maxes)
    dst_image = np.full(GUARD + cap + GUARD, fill, dtype=np.uint8)
    dst = dst_mem.alloc(dst_image.size); dst.write(dst_image)
    table_image = np.full(GUARD + 8 * (n + 1) + GUARD, fill, dtype=np.uint8)
    table = dst_mem.alloc(table_image.size); table.write(table_image)
    srcs = (d.PackSrc * n)()
    for i in range(n):
        srcs[i].base, srcs[i].bytes, srcs[i].max_bytes = src.ptr + s_off[i], lens.ptr + 8 * i, maxes[i]
    # the sum of the maxima is checked against the capacity on the host: nothing happens
    if cap:
        try:
            pack(srcs, dst.ptr + GUARD, cap - 1, table.ptr + GUARD)
        except d.D2DError as ex:
            assert ex.code == ERR_CAPACITY
        else:
            raise AssertionError("a capacity below the sum of max_bytes was accepted")
    pack(srcs, dst.ptr + GUARD, cap, table.ptr + GUARD)
    dst_mem.sync()
    want, want_table = dst_image.copy(), table_image.copy()
    if too_long is None:
        offs = np.concatenate([[0], np.cumsum(actual)]).astype("<u8")
        for i in range(n):
            o = GUARD + int(offs[i])
            want[o:o + actual[i]] = src_image[s_off[i]:s_off[i] + actual[i]]
    else:
        offs = np.full(n + 1, GAVE_UP, dtype="<u8")
    want_table[GUARD:GUARD + 8 * (n + 1)] = offs.view(np.uint8)
    got_table = table.read()
    assert np.array_equal(got_table, want_table), (case, too_long, got_table[GUARD:GUARD + 8 * (n + 1)].view("<u8")[:8])
    got = dst.read()
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{case}: {bad.size} bytes differ, the first at {bad[0] - GUARD} of {cap}"
    assert np.array_equal(src.read(), src_image)


def check_pack_empty_and_refusals(d, pack, mem):
    table = mem.alloc(16); table.write(np.full(16, 0x77, dtype=np.uint8))
    pack((d.PackSrc * 0)(), None, 0, table.ptr)
    mem.sync()
    assert table.read().view("<u8").tolist() == [0, 0x7777777777777777]
    srcs = (d.PackSrc * 1)()
    srcs[0].base, srcs[0].bytes, srcs[0].max_bytes = table.ptr, None, 4
    for bad_srcs, off in ((srcs, table.ptr), ((d.PackSrc * 0)(), None)):
        try:
            pack(bad_srcs, table.ptr, 64, off)
        except d.D2DError as ex:
            assert ex.code == ERR_PARAM
        else:
            raise AssertionError("a null pointer was accepted")
