"""flac_encode_kernel<1..8>, flac_pack_kernel and d2d_convert_stream_flac (dsd2dxd_amd/csrc/flac/d2d_flac.hip) where tests/test_gpu_flac.py does not
go: every channel count, last blocks of every residue mod 4, every Rice parameter and both sides of its thresholds, outliers at every
alignment, files of more than one pack workgroup (32 blocks) and of more sizes than one pass of its reduction (256), a caller's stream,
and the stream driver at chunks below a block and above 32 blocks and at every kind of ending.  The inputs and the proof of what they
reach are in tests/test_flac_edges_cpu.py.  Every comparison is against d2d_flac_encode_host, byte for byte: frames, result record,
frames_consumed and blocks.  Up to 16 files share a d2d_flac_encode_device call.  flac_search_kernel<1..8, LPC or not> gets its own
sweep of the channel counts (test_every_channel_count_of_the_search), against d2d_flac_encode_host_effort."""
import numpy as np
import pytest

import flac_ref as R
import test_flac_edges_cpu as E
from helpers import pack_layout, synth
from test_gpu_flac import device_encode, host_encode
from test_gpu_flac_search import device_encode as search_device_encode, host_encode as search_host_encode

gpu = pytest.mark.gpu
B = R.BLOCK
MAXF = 16                                                          # files per launch (d2d_flac.hip)


def _blocks(frames, final):
    return frames // B + (1 if final and frames % B else 0)


def compare(d, channels, depth, cases, per_call=MAXF, slack=0):
    """cases: [(label, int64 samples (frames, channels), first_block, final)], `per_call` of them in each device call"""
    files = [(R.pack_pcm(s, depth), first, final) for _, s, first, final in cases]
    want = host_encode(d, channels, depth, files)
    for at in range(0, len(files), per_call):
        got = device_encode(d, channels, depth, files[at:at + per_call], slack=slack)
        for i, g in enumerate(got):
            label, s, _, final = cases[at + i]
            w = want[at + i]
            assert g[1] == w[1], label                             # the result record
            assert g[0] == w[0], label                             # the frames
            assert g[2] == w[2] and g[3] == _blocks(s.shape[0], final), label      # frames_consumed, blocks
    return want


@gpu
@pytest.mark.parametrize("depth", E.DEPTHS)
@pytest.mark.parametrize("channels", range(1, 9))
def test_every_channel_count(engine_lib, channels, depth):
    cases = []
    for sig in ("random", "alternate", "spike"):
        for i, (frames, final) in enumerate(((2 * B + 1000, True), (B + 3, True), (B - 1, False))):
            cases.append((f"{sig} {frames}", R.signal(sig, frames, channels, depth, seed=frames + channels), 7 + i, final))
    want = compare(engine_lib, channels, depth, cases)
    assert [w[1][0] > 0 for w in want] == [True, True, False] * 3


@gpu
@pytest.mark.parametrize("depth", (16, 24))                        # the 2-byte and the 3-byte loader (20 bits is a shift of the latter)
@pytest.mark.parametrize("effort", (1, 12))
@pytest.mark.parametrize("channels", range(1, 9))
def test_every_channel_count_of_the_search(engine_lib, channels, effort, depth):
    """flac_search_kernel<1..8, LPC or not>: a whole block (partition sums by DPP rows) and a short one (by LDS adds; LPC present), the
    smallest LPC frame, and an unsearched one (the effort-0 frame), all in one call"""
    cases = []
    for sig in ("random", "alternate"):
        for i, frames in enumerate((B + 1000, 64, 15)):
            cases.append((f"{sig} {frames}", R.signal(sig, frames, channels, depth, seed=frames + channels), 7 + i, True))
    files = [(R.pack_pcm(s, depth), first, final) for _, s, first, final in cases]
    want = search_host_encode(engine_lib, channels, depth, files, effort=effort)
    got = search_device_encode(engine_lib, channels, depth, files, effort=effort)
    for (label, _, _, _), g, w in zip(cases, got, want):
        assert g[1] == w[1], label                                 # the result record
        assert g[0] == w[0], label                                 # the frames
        assert g[2] == w[2], label                                 # frames_consumed


@gpu
@pytest.mark.parametrize("channels,depth", E.SHORT_SHAPES)
def test_short_last_blocks(engine_lib, channels, depth):
    compare(engine_lib, channels, depth, [(f"{lead} + {n}", E.short_signal(channels, depth, lead, n), 3, True) for lead, n in E.SHORT_FILES])


@gpu
@pytest.mark.parametrize("depth", E.DEPTHS)
def test_k_sweep(engine_lib, depth):
    compare(engine_lib, 2, depth, [(f"{kind} {a}", E.k_sweep_signal(d, kind, a), 0, True) for d, kind, a in E.K_SWEEP if d == depth])


@gpu
@pytest.mark.parametrize("depth", (16, 24))
def test_k_edges(engine_lib, depth):
    compare(engine_lib, 3, depth, [(f"n = {n}, j = {j}", E.k_edge_signal(n, d, j), 0, True) for n, d, j in E.K_EDGES if d == depth])


@gpu
@pytest.mark.parametrize("depth", (16, 24))
def test_spikes(engine_lib, depth):
    compare(engine_lib, 2, depth, [(f"{amp} at {i} of {frames}, floor {floor}", E.spike_signal(d, frames, i, amp, floor), 0, True)
                                   for d, frames, i, amp, floor in E.SPIKES if d == depth])


def _many(shape):
    return [(f"{s[2]} x 4096 + {s[3]}", E.many_blocks_signal(s), s[4], s[5]) for s in E.MANY_BLOCKS if s[:2] == shape]


@gpu
def test_many_blocks_share_a_call(engine_lib):
    """files of 0, 1 and 31 .. 300 blocks in ONE call: the grid is the largest file's, so most pack and encode workgroups of the small
    files have nothing to do and must return; later pack workgroups find their offset from the sizes in front of them"""
    cases = _many((1, 16))
    assert len(cases) == 10 and max(_blocks(s.shape[0], f) for _, s, _, f in cases) == 300
    want = compare(engine_lib, 1, 16, cases)
    zero = [w for (_, s, _, f), w in zip(cases, want) if _blocks(s.shape[0], f) == 0]
    assert len(zero) == 1 and zero[0][1] == (0, 0, 0) and zero[0][0] == b""
    compare(engine_lib, 2, 24, _many((2, 24)))


@gpu
def test_many_blocks_behind_a_guard(engine_lib):
    """the same call with 4096 bytes of out buffer behind every file's capacity: device_encode asserts that nothing behind bytes_out
    was written, here well past the bound too"""
    compare(engine_lib, 1, 16, _many((1, 16)), slack=4096)


@gpu
def test_many_blocks_across_two_launches(engine_lib):
    """17 files: one more than a launch carries descriptors for, so the call is two launches over one workspace"""
    cases = _many((1, 16))
    small = [c for c in cases if _blocks(c[1].shape[0], c[3]) <= 65]
    cases = cases + small[::-1][:17 - len(cases)]                  # (the 17th file, alone in the second launch: 31 blocks)
    assert len(cases) == 17 and _blocks(cases[16][1].shape[0], cases[16][3]) > 0
    compare(engine_lib, 1, 16, cases, per_call=17)


@gpu
def test_a_callers_stream(engine_lib):
    """PCM uploaded (from pinned memory, asynchronously) and encoded on a non-default stream whose handle goes in as hip_stream; the result
    is read after synchronising that stream alone"""
    import torch
    d, ch, depth = engine_lib, 2, 24
    shapes = ((40 * B + 123, True, 0), (B, True, 0x7FF), (5, True, 1), (B - 1, False, 0))
    pcms = [R.pack_pcm(R.varying(n, ch, depth, seed=i), depth) for i, (n, _, _) in enumerate(shapes)]
    want = host_encode(d, ch, depth, [(p, first, final) for p, (_, final, first) in zip(pcms, shapes)])
    s = torch.cuda.Stream()
    assert s.cuda_stream != 0 and s != torch.cuda.default_stream()
    ios = (d.FlacIO * len(shapes))()
    keep, ws = [], 0
    with torch.cuda.stream(s):
        rec = torch.full((16 * len(shapes),), 0xEE, dtype=torch.uint8, device="cuda")
        for i, (p, (n, final, first)) in enumerate(zip(pcms, shapes)):
            pinned = torch.from_numpy(p).pin_memory()
            tp = pinned.to("cuda", non_blocking=True)
            cap = d.flac_bound_bytes(ch, depth, n, final)
            to = torch.full((max(cap, 16),), 0xA5, dtype=torch.uint8, device="cuda")
            assert tp.data_ptr() % 16 == 0 and to.data_ptr() % 16 == 0
            keep.append((pinned, tp, to))
            ios[i].pcm, ios[i].frames, ios[i].first_block, ios[i].final = tp.data_ptr(), n, first, int(final)
            ios[i].out, ios[i].out_capacity_bytes, ios[i].result = to.data_ptr(), cap, rec.data_ptr() + 16 * i
            ws += d.flac_workspace_bytes(ch, depth, n, final)
        tw = torch.zeros(max(ws, 16), dtype=torch.uint8, device="cuda")
        d.flac_encode_device(ch, depth, ios, tw.data_ptr(), ws, stream=s.cuda_stream)
        host_rec = torch.empty(rec.shape, dtype=torch.uint8).pin_memory()
        host_out = [torch.empty(k[2].shape, dtype=torch.uint8).pin_memory() for k in keep]
        host_rec.copy_(rec, non_blocking=True)
        for h, k in zip(host_out, keep):
            h.copy_(k[2], non_blocking=True)
    s.synchronize()                                                # this stream only: no device-wide wait anywhere above
    r = host_rec.numpy().view(np.uint64).reshape(len(shapes), 2)
    for i, w in enumerate(want):
        bytes_out, mm = int(r[i, 0]), int(r[i, 1])
        o = host_out[i].numpy()
        assert (bytes_out, mm & 0xFFFFFFFF, mm >> 32) == w[1], i
        assert o[:bytes_out].tobytes() == w[0], i
        assert (o[bytes_out:] == 0xA5).all(), i
        assert ios[i].frames_consumed == w[2] and ios[i].blocks == _blocks(shapes[i][0], shapes[i][1]), i
    torch.cuda.synchronize()


# ---- the stream twin ------------------------------------------------------------------------------------------------------------------
# DSD64 -> 88.2 kHz: one frame per 4 input bytes per channel.  (engine shape) x (bytes per channel of the stream, of a chunk)
ENGINES = (dict(channels=1, bit_depth=16), dict(channels=2, bit_depth=24), dict(channels=3, bit_depth=20))
STREAMS = {
    "quarter-block-chunks": (4 * (2 * B + 2048), 4 * 1024),       # ten chunks of 1024 frames: three calls in four encode nothing
    "exactly-two-blocks": (4 * 2 * B, 4 * 3072),                   # ends on a block boundary: no short frame
    "under-one-block": (4 * 3072, 4 * 4096),
    "empty": (0, 4 * 4096),
    "one-chunk-of-33-blocks": (4 * (33 * B + 1024), 4 * 34 * B),
}


def _stream_kw(channels, bit_depth):
    return dict(dsd_rate=1, output_rate=88200, channels=channels, fmt="P", endianness="L", block_size=4096, filter="E",
                bit_depth=bit_depth, dither="T", seed=5)


@gpu
@pytest.mark.parametrize("stream", STREAMS)
@pytest.mark.parametrize("shape", ENGINES, ids=lambda s: f"{s['channels']}ch{s['bit_depth']}")
def test_stream_twin(engine_lib, oracle_mod, shape, stream):
    d, ch, depth = engine_lib, shape["channels"], shape["bit_depth"]
    nbytes, chunk = STREAMS[stream]
    kw = _stream_kw(ch, depth)
    chans = [synth("sine" if c % 2 == 0 else "pink", nbytes, seed=30 + c, amp=0.352 if c % 2 == 0 else 0.098) for c in range(ch)]
    fb = ch * (2 if depth == 16 else 3)
    if nbytes:
        ref, rf = oracle_mod.Oracle(**kw).translate(pack_layout(chans, "P", 4096))
        ref = ref[:rf * fb]
    else:
        ref, rf = np.zeros(0, dtype=np.uint8), 0
    assert rf == nbytes // 4
    want, res, used = d.flac_encode_host(ch, depth, ref, first_block=0, final=True)
    assert used == rf
    pos, reads = [0], []

    def read(cap):
        assert cap == chunk
        a = pos[0]
        b = min(nbytes, a + cap)
        pos[0] = b
        reads.append(b - a)
        return pack_layout([c[a:b] for c in chans], "P", 4096).tobytes() if b > a else b""

    out, prog = [], []
    e = d.Engine(**kw)
    stats = e.convert_stream_flac(read, out.append, total_bytes_per_channel=nbytes, chunk_bytes_per_channel=chunk, progress=prog.append)
    e.close()
    assert b"".join(out) == want
    blocks = _blocks(rf, True)
    assert (stats.samples_per_channel, stats.blocks, stats.min_frame_bytes, stats.max_frame_bytes) == \
           (rf, blocks, res.min_frame_bytes, res.max_frame_bytes)
    assert all(o[:2] == b"\xff\xf8" for o in out)                  # every write begins with a frame
    assert prog[-1] == 100.0 and all(p < 100.0 for p in prog[:-1]) and prog == sorted(prog)
    assert reads[-1] == 0 and sum(reads) == nbytes
    if stream == "quarter-block-chunks":
        assert len(reads) == 11 and len(out) == 3 and blocks == 3  # ten calls, three of them with a block to write
    if stream == "exactly-two-blocks":
        assert rf == 2 * B and rf % B == 0 and blocks == 2
        got = b"".join(out)
        sizes = R.decode(got, ch, depth)[1]
        assert len(sizes) == 2 and got[2] >> 4 == 0xC and got[sizes[0] + 2] >> 4 == 0xC      # the last frame too: block-size code 4096
    if stream == "under-one-block":
        assert 0 < rf < B and blocks == 1 and len(out) == 1 and want[2] >> 4 == 0x7
    if stream == "empty":
        assert want == b"" and out == [] and prog == [100.0]
        assert (stats.samples_per_channel, stats.blocks, stats.min_frame_bytes, stats.max_frame_bytes) == (0, 0, 0, 0)
    if stream == "one-chunk-of-33-blocks":
        assert len(reads) == 2 and blocks == 34 and len(out) == 1
