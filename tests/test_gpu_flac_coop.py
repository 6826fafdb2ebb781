"""d2d_flac_verify_device_method (include/dsd2dxd_amd.h): the cooperative verify kernel, one workgroup per frame, beside the serial
one.  For both methods the device's records AND its counts of who decided each block (d2d_flac_verify_stats) must be the host twin's
on the downloaded bytes; tests/test_flac_coop_cpu.py pins the twin to the serial parser, flip by flip.  Ragged batches of more than
sixteen files on a caller's stream with nothing between encode and verify, the crafted damage of tests/test_flac_verify_cpu.py, the
effort-12 bit-flip corpus one file per flipped frame, frame numbers across every UTF-8 length, frame starts at all four byte
alignments, the largest frame the kernel's LDS must hold and the smallest ones, and what a call may touch."""
import numpy as np
import pytest

import flac_ref as R
from test_flac_coop_cpu import AUTO, COOP, FLIP_FIRST, FLIP_N, SERIAL, flip_corpus, flip_frames, largest_frame_signal, wrong_size_tables
from test_flac_verify_cpu import (BAD_NONE, BAD_SAMPLES, BLOCK, CRAFT_CH, CRAFT_DEPTH, CRAFT_FIRST, EFFORTS, LENGTHS, MUTATIONS, NONE, clean, craft_stream,
                                  damaged, make_signal, mutations, nblocks)
from test_gpu_containment import Arena, describe, fill_bytes, violations
from test_gpu_flac_search import _dev, _host
from test_gpu_flac_verify import CHECK_BYTES, Batch, crafted_batch, records

gpu = pytest.mark.gpu
STATS_BYTES = 8
METHODS = (SERIAL, COOP)


def stats_of(t, n):
    return [tuple(int(v) for v in t[STATS_BYTES * i:STATS_BYTES * (i + 1)].view(np.uint32)) for i in range(n)]


def verify(b, method, stream=None):
    """a verify call of Batch b at `method` into records and stats of its own; returns the two device tensors"""
    n = len(b.files)
    chk, st = _dev(np.full(CHECK_BYTES * n, 0xDD, dtype=np.uint8)), _dev(np.full(STATS_BYTES * n, 0xCC, dtype=np.uint8))
    b.d.flac_verify_device(b.ch, b.depth, b.ios, b.ws.data_ptr(), b.ws_bytes, chk.data_ptr(), stream=stream, method=method, stats_ptr=st.data_ptr())
    return chk, st


def host(b, method):
    """the host twin at `method` on the PCM, the bytes and the size tables the device holds: ([records], [stats])"""
    recs, stats = [], []
    for i, (pcm, first, final) in enumerate(b.files):
        out, sizes = b.frames(i)
        pcm = _host(b.pcm[i])[:pcm.size].copy()
        st = b.d.FlacVerifyStats()
        recs.append(b.d.flac_verify_host(b.ch, b.depth, pcm, out, first_block=first, final=final, sizes=sizes, method=method, stats=st).as_tuple())
        stats.append(st.as_tuple())
    return recs, stats


def both_methods(b, stream=None, sync=None):
    """SERIAL and COOP enqueued one behind the other; {method: ([records], [stats])} of the device, each compared with the host twin's"""
    pending = {m: verify(b, m, stream) for m in METHODS}
    if sync:
        sync()
    out = {}
    for m, (chk, st) in pending.items():
        got = (records(_host(chk), len(b.files)), stats_of(_host(st), len(b.files)))
        assert got == host(b, m), (m, got)
        out[m] = got
    assert out[SERIAL][0] == out[COOP][0]
    return out


# ---- clean, ragged batches ----------------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("depth", (16, 20, 24))
@pytest.mark.parametrize("channels", (1, 2, 3, 8))
@pytest.mark.parametrize("effort", EFFORTS)
def test_clean_ragged_batches_on_a_callers_stream(engine_lib, effort, channels, depth):
    """twenty files -- the ten lengths twice, the second time not final and numbered from elsewhere -- in one call: two groups of launches;
    encode, the serial verify and the cooperative verify enqueued on a non-blocking stream with no synchronisation between them"""
    import torch
    files = []
    for rnd in range(2):
        for i, n in enumerate(LENGTHS):
            x = make_signal((i + channels + depth + rnd) % 5, n, channels, depth, 7 * i + channels + rnd)
            files.append((R.pack_pcm(x, depth), 126 + i + 1900 * rnd, rnd == 0))
    b = Batch(engine_lib, channels, depth, files)
    assert len(files) > 16
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    b.encode(effort, stream=s.cuda_stream)
    got = both_methods(b, stream=s.cuda_stream, sync=s.synchronize)
    want = [clean(n if final else n // BLOCK * BLOCK, nblocks(n) if final else n // BLOCK) for final in (True, False) for n in LENGTHS]
    assert got[COOP][0] == want, got[COOP][0]
    assert got[COOP][1] == [(w[1], 0) for w in want] and got[SERIAL][1] == [(0, w[1]) for w in want]     # every block by the fast path


# ---- damage ------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def crafted(engine_lib):
    x, pcm, frames, sizes = craft_stream(engine_lib)
    a, b = sizes[0], sizes[0] + sizes[1]
    return dict(x=x, pcm=pcm, frames=frames, sizes=sizes, muts=mutations(frames[a:b])[0])


@gpu
@pytest.mark.parametrize("name", MUTATIONS)
def test_crafted_mutations_on_the_device(engine_lib, crafted, name):
    import torch
    d, c = engine_lib, crafted
    b = crafted_batch(d, c)
    out = np.frombuffer(damaged(c, name), dtype=np.uint8)
    b.out[1][:out.size] = torch.from_numpy(out.copy()).cuda()
    got = both_methods(b)
    reason = c["muts"][name][1]
    rec = got[COOP][0]
    assert rec[1][:4] == (c["x"].shape[0] - BLOCK, 3, 1, 1) and rec[1][4] in (reason if isinstance(reason, tuple) else (reason,)), rec[1]
    assert rec[0] == clean(BLOCK + 5, 2) and rec[2] == clean(BLOCK + 5, 2)
    assert got[COOP][1] == [(2, 0), (2, 1), (2, 0)]


@gpu
def test_wrong_size_entries_and_changed_pcm_on_the_device(engine_lib, crafted):
    import torch
    d, c = engine_lib, crafted
    for sizes, bad in wrong_size_tables(c):
        b = crafted_batch(d, c)
        b.ws[b.ws_at[1]:b.ws_at[1] + 12] = torch.from_numpy(np.array(sizes, dtype=np.uint32).view(np.uint8).copy()).cuda()
        got = both_methods(b)
        assert got[COOP][0][1][:4] == (BLOCK, 3, bad, 1) and got[COOP][1][1] == (1, 2), (sizes, got[COOP])
    for frame_index, channel in ((BLOCK + 17, 1), (2 * BLOCK + 99, 0)):
        b = crafted_batch(d, c)
        b.pcm[1][(frame_index * CRAFT_CH + channel) * 3] ^= 1
        block = frame_index // BLOCK
        got = both_methods(b)
        assert got[COOP][0][1] == (c["x"].shape[0] - (BLOCK, BLOCK, 100)[block], 3, 1, block, BAD_SAMPLES) and got[COOP][1][1] == (2, 1)


class FrameFiles:
    """one-block files that share one PCM, each frame given as bytes: `out` slots, size tables and result records are written as an
    encode call would have left them, so that thousands of damaged frames take one verify call"""

    def __init__(self, d, channels, depth, pcm, n, first, frames):
        self.d, self.ch, self.depth, self.n_files = d, channels, depth, len(frames)
        self.pcm = _dev(pcm)
        wsb = d.flac_workspace_bytes(channels, depth, n, True)
        cap = (d.flac_bound_bytes(channels, depth, n, True) + 15) // 16 * 16
        out, ws, rec = np.full(cap * len(frames), 0xA5, dtype=np.uint8), np.zeros(wsb * len(frames), dtype=np.uint8), np.zeros(16 * len(frames), dtype=np.uint8)
        for i, f in enumerate(frames):
            out[cap * i:cap * i + len(f)] = np.frombuffer(f, dtype=np.uint8)
            ws[wsb * i:wsb * i + 4] = np.array([len(f)], dtype=np.uint32).view(np.uint8)
            rec[16 * i:16 * i + 8] = np.array([len(f)], dtype=np.uint64).view(np.uint8)
        self.out, self.ws, self.rec = _dev(out), _dev(ws), _dev(rec)
        self.ios = (d.FlacIO * len(frames))()
        for i in range(len(frames)):
            io = self.ios[i]
            io.pcm, io.frames, io.first_block, io.final = self.pcm.data_ptr(), n, first, 1
            io.out, io.out_capacity_bytes, io.result = self.out.data_ptr() + cap * i, cap, self.rec.data_ptr() + 16 * i

    def verify(self, method):
        n = self.n_files
        chk, st = _dev(np.full(CHECK_BYTES * n, 0xDD, dtype=np.uint8)), _dev(np.full(STATS_BYTES * n, 0xCC, dtype=np.uint8))
        self.d.flac_verify_device(self.ch, self.depth, self.ios, self.ws.data_ptr(), self.ws.numel(), chk.data_ptr(), method=method, stats_ptr=st.data_ptr())
        return records(_host(chk), n), stats_of(_host(st), n)


@gpu
def test_the_bit_flip_corpus_of_the_effort_12_frame(engine_lib):
    """every single-bit flip of the effort-12 frame with both CRCs repaired, and the frame itself: one file each, one call per method"""
    d = engine_lib
    pcm, frame = flip_frames(d)[12]
    frames = [frame] + [f for _, f in flip_corpus(frame, True)]
    assert len(frames) > 1000
    want, want_st = [], []
    for f in frames:
        st = d.FlacVerifyStats()
        want.append(d.flac_verify_host(2, 16, pcm, f, first_block=FLIP_FIRST, sizes=[len(f)], method=COOP, stats=st).as_tuple())
        want_st.append(st.as_tuple())
    assert want[0] == clean(FLIP_N, 1) and want_st[0] == (1, 0) and all(w[4] != BAD_NONE and s == (0, 1) for w, s in zip(want[1:], want_st[1:]))
    ff = FrameFiles(d, 2, 16, pcm, FLIP_N, FLIP_FIRST, frames)
    got, got_st = ff.verify(COOP)
    wrong = [i for i in range(len(frames)) if got[i] != want[i] or got_st[i] != want_st[i]]
    assert not wrong, (len(wrong), wrong[:5], [(got[i], want[i], got_st[i]) for i in wrong[:5]])
    got, got_st = ff.verify(SERIAL)
    assert got == want and got_st == [(0, 1)] * len(frames)


# ---- positions -----------------------------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("effort", EFFORTS)
def test_frame_numbers_across_the_utf8_lengths(engine_lib, effort):
    """three blocks from just below 2^7, 2^11, 2^16, 2^21 and 2^26: the header grows by a byte inside each file, and with it every later
    bit position and the alignment of the frames behind"""
    firsts = [(1 << k) - 1 for k in (7, 11, 16, 21, 26)] + [0, (1 << 31) - 3]
    sigs = [make_signal(i % 5, 2 * BLOCK + 77, 2, 24, i) for i in range(len(firsts))]
    b = Batch(engine_lib, 2, 24, [(R.pack_pcm(x, 24), first, True) for x, first in zip(sigs, firsts)])
    b.encode(effort)
    got = both_methods(b)
    assert got[COOP][0] == [clean(2 * BLOCK + 77, 3)] * len(firsts) and got[COOP][1] == [(3, 0)] * len(firsts)
    # the header's length does change inside each of the first five files: 4 + the UTF-8 bytes of the frame number + the CRC-8
    def utf8_bytes(lead):
        ones = 8 - int(lead ^ 0xFF).bit_length()
        return ones or 1

    for i, k in enumerate((1, 2, 3, 4, 5)):
        out, sizes = b.frames(i)
        assert (utf8_bytes(int(out[4])), utf8_bytes(int(out[int(sizes[0]) + 4]))) == (k, k + 1), (i, out[4], out[int(sizes[0]) + 4])


@gpu
@pytest.mark.parametrize("effort", EFFORTS)
def test_frame_starts_at_all_four_byte_alignments(engine_lib, effort):
    """noise of varying width: frames of every size modulo 4, so frames start at every alignment of `out` -- asserted on the batch"""
    sigs = [R.varying(6 * BLOCK + 11 * i, 2, 16, 40 + i) for i in range(3)]
    b = Batch(engine_lib, 2, 16, [(R.pack_pcm(x, 16), 0, True) for x in sigs])
    b.encode(effort)
    got = both_methods(b)
    starts = set()
    for i in range(3):
        sizes = b.frames(i)[1]
        starts |= {int(v) % 4 for v in np.concatenate([[0], np.cumsum(sizes.astype(np.int64))[:-1]])}
    assert starts == {0, 1, 2, 3}, starts
    assert got[COOP][0] == [clean(x.shape[0], nblocks(x.shape[0])) for x in sigs] and got[COOP][1] == [(nblocks(x.shape[0]), 0) for x in sigs]


@gpu
def test_the_largest_and_the_smallest_frames(engine_lib):
    d = engine_lib
    x, effort = largest_frame_signal()                       # tests/test_flac_coop_cpu.py asserts its frame fills 0.9 of the bound
    b = Batch(d, 8, 24, [(R.pack_pcm(x, 24), 0, True), (R.pack_pcm(make_signal(1, BLOCK + 3, 8, 24, 2), 24), 5, True)])
    b.encode(effort)
    got = both_methods(b)
    assert int(b.frames(0)[1][0]) >= 0.9 * R.frame_bound(8, 24, BLOCK)
    assert got[COOP][0] == [clean(BLOCK, 1), clean(BLOCK + 3, 2)] and got[COOP][1] == [(1, 0), (2, 0)]
    for eff in EFFORTS:                                      # digital silence, and the verbatim frames of one and two samples
        shapes = (BLOCK, 1, 2, 2 * BLOCK + 1)
        b = Batch(d, 1, 16, [(R.pack_pcm(np.zeros((n, 1), dtype=np.int64) + (n < 3) * 1234, 16), 0, True) for n in shapes])
        b.encode(eff)
        got = both_methods(b)
        assert got[COOP][0] == [clean(n, nblocks(n)) for n in shapes] and got[COOP][1] == [(nblocks(n), 0) for n in shapes]


# ---- what a call touches --------------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("complement", (False, True))
def test_a_method_call_writes_only_its_records_its_stats_and_the_workspace(engine_lib, complement):
    """pcm, out, workspace, result records, check records and stats each in an arena between guards, two complementary fills.  After a
    call at either method out, pcm and the result records are what the encode call left, nothing outside the workspace, the check records
    and the stats changed, and what was written is the host twin's answer under both fills: nothing it depends on was read from outside.
    A refused call -- an unknown method among them -- changed nothing at all"""
    d, ch, depth = engine_lib, 2, 24
    shapes = ((BLOCK + 1000, True, 3), (0, True, 0), (2 * BLOCK + 100, False, 0x7FF), (17, True, 0))
    pcms = [R.pack_pcm(make_signal(i % 5, n, ch, depth, i) if n else np.zeros((0, 2), dtype=np.int64), depth) for i, (n, _, _) in enumerate(shapes)]
    caps = [d.flac_bound_bytes(ch, depth, n, f) for n, f, _ in shapes]
    wss = sum(d.flac_workspace_bytes(ch, depth, n, f) for n, f, _ in shapes)
    a_in, a_out, a_ws, a_rec = Arena([p.size for p in pcms]), Arena(caps), Arena([wss]), Arena([16 * len(shapes)])
    a_chk, a_st = Arena([CHECK_BYTES * len(shapes)]), Arena([STATS_BYTES * len(shapes)])
    arenas = (a_in, a_out, a_ws, a_rec, a_chk, a_st)
    names = ("pcm", "out", "workspace", "result records", "check records", "stats")
    fills = [fill_bytes(a.total, complement).copy() for a in arenas]
    for s, p in zip(a_in.starts, pcms):
        fills[0][s:s + p.size] = p
    tensors = tuple(_dev(f) for f in fills)
    t_in, t_out, t_ws, t_rec, t_chk, t_st = tensors
    ios = (d.FlacIO * len(shapes))()
    for i, (n, final, first) in enumerate(shapes):
        ios[i].pcm, ios[i].frames, ios[i].first_block, ios[i].final = t_in.data_ptr() + a_in.starts[i], n, first, int(final)
        ios[i].out, ios[i].out_capacity_bytes = t_out.data_ptr() + a_out.starts[i], caps[i]
        ios[i].result = t_rec.data_ptr() + a_rec.starts[0] + 16 * i
    ws_ptr, chk_ptr, st_ptr = t_ws.data_ptr() + a_ws.starts[0], t_chk.data_ptr() + a_chk.starts[0], t_st.data_ptr() + a_st.starts[0]
    d.flac_encode_device(ch, depth, ios, ws_ptr, wss, effort=12)
    before = [_host(t).copy() for t in tensors]

    for bad, code in ((dict(method=3), -1), (dict(method=0xFFFFFFFF), -1), (dict(st=st_ptr + 2), -1), (dict(depth=12), -1), (dict(wss=wss - 1), -20), (dict(chk=0), -1)):
        with pytest.raises(d.D2DError) as ei:
            d.flac_verify_device(ch, bad.get("depth", depth), ios, ws_ptr, bad.get("wss", wss), bad.get("chk", chk_ptr), method=bad.get("method", COOP),
                                 stats_ptr=bad.get("st", st_ptr))
        assert ei.value.code == code, bad
        for t, f, name in zip(tensors, before, names):
            assert np.array_equal(_host(t), f), f"refused call {bad}: the {name} arena changed"

    want_chk, want_st = {}, {}
    for method in (COOP, SERIAL, AUTO):
        d.flac_verify_device(ch, depth, ios, ws_ptr, wss, chk_ptr, method=method, stats_ptr=st_ptr)
        after = [_host(t) for t in tensors]
        for k in (0, 1, 3):
            assert np.array_equal(after[k], before[k]), f"method {method}: the {names[k]} arena changed"
        v = violations(a_ws, after[2], fills[2], [after[2][a_ws.starts[0]:a_ws.end(0)]])
        assert not v, f"method {method}, workspace: " + describe(v)
        chk, st = np.zeros(len(shapes) * CHECK_BYTES, dtype=np.uint8), np.zeros(len(shapes) * STATS_BYTES, dtype=np.uint8)
        for i, (n, final, _) in enumerate(shapes):
            used = n if final else n // BLOCK * BLOCK
            chk[CHECK_BYTES * i:CHECK_BYTES * i + 8] = np.array([used], dtype=np.uint64).view(np.uint8)
            chk[CHECK_BYTES * i + 8:CHECK_BYTES * (i + 1)] = np.array([nblocks(used), 0, NONE, BAD_NONE], dtype=np.uint32).view(np.uint8)
            st[STATS_BYTES * i:STATS_BYTES * (i + 1)] = np.array([0, nblocks(used)] if method == SERIAL else [nblocks(used), 0], dtype=np.uint32).view(np.uint8)
        v = violations(a_chk, after[4], fills[4], [chk])
        assert not v, f"method {method}, check records: " + describe(v)
        v = violations(a_st, after[5], fills[5], [st])
        assert not v, f"method {method}, stats: " + describe(v)
    # stats = NULL: the stats arena stays as the last call left it
    last = _host(t_st).copy()
    d.flac_verify_device(ch, depth, ios, ws_ptr, wss, chk_ptr, method=COOP)
    assert np.array_equal(_host(t_st), last)
