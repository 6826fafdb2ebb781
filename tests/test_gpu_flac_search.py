"""FLAC effort 1 on the GPU (include/dsd2dxd_amd.h, "EFFORTS"): d2d_flac_encode_device_effort, d2d_convert_stream_flac_effort and the
CLI's --flac-effort against d2d_flac_encode_host_effort -- the sink's own encoder, pinned to the definition by
tests/test_flac_search_cpu.py -- byte for byte.  The inputs are that file's CASES, so its assertion that they force every predictor
order, partition order, channel assignment and tie covers what runs here; the cases of one (channels, depth) go through one call."""
import os
import subprocess

import numpy as np
import pytest

import flac_ref as R
import flac_search_ref as S
from helpers import pack_layout, synth, write_dsf
from test_flac_search_cpu import CASES, stereo, step, walk
from test_gpu_containment import Arena, describe, fill_bytes, violations

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "dsd2dxd_amd", "dsd2dxd_amd_cli")
SEARCH = 1


def _dev(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    assert t.data_ptr() % 16 == 0
    return t


def _host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


def host_encode(d, channels, depth, files, effort=SEARCH):
    """files: [(pcm uint8 array, first_block, final)] -> [(frame bytes, (bytes_out, min, max), frames consumed)]"""
    out = []
    for pcm, first, final in files:
        b, res, used = d.flac_encode_host(channels, depth, pcm, first_block=first, final=final, effort=effort)
        out.append((b, (res.bytes_out, res.min_frame_bytes, res.max_frame_bytes), used))
    return out


def device_encode(d, channels, depth, files, effort=SEARCH):
    """one d2d_flac_encode_device_effort call over `files`, each in buffers of its own; the same shape of result as host_encode"""
    fb = channels * (2 if depth == 16 else 3)
    n = len(files)
    ios = (d.FlacIO * n)()
    keep, ws = [], 0
    rec = _dev(np.full(16 * n, 0xEE, dtype=np.uint8))
    for i, (pcm, first, final) in enumerate(files):
        frames = pcm.size // fb
        cap = d.flac_bound_bytes(channels, depth, frames, final)
        tp, to = _dev(pcm if pcm.size else np.zeros(16, dtype=np.uint8)), _dev(np.full(max(cap, 16), 0xA5, dtype=np.uint8))
        keep.append((tp, to))
        ios[i].pcm, ios[i].frames, ios[i].first_block, ios[i].final = tp.data_ptr(), frames, first, int(final)
        ios[i].out, ios[i].out_capacity_bytes, ios[i].result = to.data_ptr(), cap, rec.data_ptr() + 16 * i
        ws += d.flac_workspace_bytes(channels, depth, frames, final)
    tw = _dev(np.zeros(max(ws, 16), dtype=np.uint8))
    d.flac_encode_device(channels, depth, ios, tw.data_ptr(), ws, effort=effort)
    r = _host(rec).view(np.uint64).reshape(n, 2)
    got = []
    for i in range(n):
        bytes_out, mm = int(r[i, 0]), int(r[i, 1])
        o = _host(keep[i][1])
        assert (o[bytes_out:] == 0xA5).all(), f"file {i}: bytes behind bytes_out were written"
        got.append((o[:bytes_out].tobytes(), (bytes_out, mm & 0xFFFFFFFF, mm >> 32), ios[i].frames_consumed))
    return got


GROUPS = sorted({(c["samples"].shape[1], c["depth"]) for c in CASES})


@gpu
@pytest.mark.parametrize("channels,depth", GROUPS, ids=lambda v: str(v))
def test_the_cpu_cases_equal_the_host_encoder(engine_lib, channels, depth):
    mine = [c for c in CASES if (c["samples"].shape[1], c["depth"]) == (channels, depth)]
    assert any(16 <= c["samples"].shape[0] for c in mine)
    files = [(R.pack_pcm(c["samples"], depth), c["first_block"], c["final"]) for c in mine]
    want = host_encode(engine_lib, channels, depth, files)
    got = device_encode(engine_lib, channels, depth, files)
    for c, g, w in zip(mine, got, want):
        assert g[1] == w[1], c["name"]                              # the result record
        assert g[0] == w[0], c["name"]                              # the frames
        assert g[2] == w[2], c["name"]                              # frames_consumed


def test_the_groups_reach_from_16_samples_to_two_blocks_and_a_short_one():
    lengths = {c["samples"].shape[0] for c in CASES}
    assert {15, 16, 17, 32, 1024, 4096, 4096 + 1000, 2 * 4096 + 1000, 4095} <= lengths
    assert {ch for ch, _ in GROUPS} == {1, 2, 3, 8} and {d for _, d in GROUPS} == {16, 20, 24}


# (frames, final, first_block): more files than one launch carries descriptors for (16), whole and short blocks, nothing at all
RAGGED = [(0, False, 9), (1000, False, 0), (4096, False, 0x7F), (2 * 4096 + 17, True, 1000), (4096 + 2048, True, 77), (16, True, 0x7FF),
          (4096 + 15, True, 5), (4095, True, 0), (1024, True, 3)] * 2 + [(4096, True, 0)]


@gpu
def test_ragged_batch_and_determinism(engine_lib):
    assert len(RAGGED) > 16
    sigs = []
    for i, (n, _, _) in enumerate(RAGGED):
        s = stereo(n, 24, S.MODES[i % 4], 40 + i) if n else np.zeros((0, 2), dtype=np.int64)
        if n >= 4096 and i % 3 == 0:
            s[:4096] += step(4096, 2, 24, 1 + i % 6, i)             # partition orders vary over the batch as well
        sigs.append(R._clip(s, 24))
    files = [(R.pack_pcm(s, 24), first, final) for s, (_, final, first) in zip(sigs, RAGGED)]
    want = host_encode(engine_lib, 2, 24, files)
    got = device_encode(engine_lib, 2, 24, files)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (i, RAGGED[i])
    assert got[0][1] == (0, 0, 0) and got[1][1] == (0, 0, 0)
    assert device_encode(engine_lib, 2, 24, files) == got          # the same call again: the same bytes


@gpu
def test_effort_0_through_the_new_entry_is_the_old_kernel(engine_lib):
    files = [(R.pack_pcm(R.signal("sine", 4096 + 100, 2, 24), 24), 0, True)]
    assert device_encode(engine_lib, 2, 24, files, effort=0) == host_encode(engine_lib, 2, 24, files, effort=0)


@gpu
@pytest.mark.parametrize("complement", (False, True))
def test_a_call_writes_only_what_it_reports(engine_lib, complement):
    """as tests/test_gpu_flac.py at effort 0: out buffers back to back with exact capacities, the workspace and the result records
    between guards, two complementary fills.  After a successful effort-1 call only [0, bytes_out) of each out, the records and the
    inside of the workspace differ from the fill; after a refused call -- an unknown effort, a capacity a byte short -- nothing does"""
    d, ch, depth = engine_lib, 2, 24
    shapes = ((4096 + 1000, True, 3), (0, True, 0), (2 * 4096 + 100, False, 0x7FF), (1024, True, 1), (17, True, 0))
    pcms = [R.pack_pcm(stereo(n, depth, S.MODES[(i + 1) % 4], i) if n else np.zeros((0, 2), dtype=np.int64), depth) for i, (n, _, _) in enumerate(shapes)]
    caps = [d.flac_bound_bytes(ch, depth, n, f) for n, f, _ in shapes]
    wss = sum(d.flac_workspace_bytes(ch, depth, n, f) for n, f, _ in shapes)
    a_in, a_out, a_ws, a_rec = Arena([p.size for p in pcms]), Arena(caps), Arena([wss]), Arena([16 * len(shapes)])
    fills = [fill_bytes(a.total, complement).copy() for a in (a_in, a_out, a_ws, a_rec)]
    for s, p in zip(a_in.starts, pcms):
        fills[0][s:s + p.size] = p
    t_in, t_out, t_ws, t_rec = (_dev(f) for f in fills)

    def ios(short=None):
        x = (d.FlacIO * len(shapes))()
        for i, (n, final, first) in enumerate(shapes):
            x[i].pcm, x[i].frames, x[i].first_block, x[i].final = t_in.data_ptr() + a_in.starts[i], n, first, int(final)
            x[i].out, x[i].out_capacity_bytes = t_out.data_ptr() + a_out.starts[i], caps[i] - (1 if short == i else 0)
            x[i].result = t_rec.data_ptr() + a_rec.starts[0] + 16 * i
        return x

    def unchanged(what):
        for t, f, name in ((t_in, fills[0], "pcm"), (t_out, fills[1], "out"), (t_ws, fills[2], "workspace"), (t_rec, fills[3], "records")):
            assert np.array_equal(_host(t), f), f"{what}: the {name} arena changed"

    with pytest.raises(d.D2DError) as ei:
        d.flac_encode_device(ch, depth, ios(), t_ws.data_ptr() + a_ws.starts[0], wss, effort=2)
    assert ei.value.code == -1 and "effort" in ei.value.message
    unchanged("unknown effort")
    with pytest.raises(d.D2DError) as ei:
        d.flac_encode_device(ch, depth, ios(short=2), t_ws.data_ptr() + a_ws.starts[0], wss, effort=SEARCH)
    assert ei.value.code == -20
    unchanged("capacity one byte short")

    want = host_encode(d, ch, depth, [(p, first, final) for p, (_, final, first) in zip(pcms, shapes)])
    d.flac_encode_device(ch, depth, ios(), t_ws.data_ptr() + a_ws.starts[0], wss, effort=SEARCH)
    got_out, got_ws, got_rec = _host(t_out), _host(t_ws), _host(t_rec)
    expect = []
    for i, (b, _, _) in enumerate(want):
        w = fills[1][a_out.starts[i]:a_out.end(i)].copy()
        w[:len(b)] = np.frombuffer(b, dtype=np.uint8)
        expect.append(w if caps[i] else None)
    v = violations(a_out, got_out, fills[1], expect)
    assert not v, describe(v)
    v = violations(a_ws, got_ws, fills[2], [got_ws[a_ws.starts[0]:a_ws.end(0)]])       # the inside is the call's own
    assert not v, "workspace: " + describe(v)
    rec = np.zeros(len(shapes) * 2, dtype=np.uint64)
    for i, (_, r, _) in enumerate(want):
        rec[2 * i], rec[2 * i + 1] = r[0], r[1] | (r[2] << 32)
    v = violations(a_rec, got_rec, fills[3], [rec.view(np.uint8)])
    assert not v, "records: " + describe(v)
    assert np.array_equal(_host(t_in), fills[0]), "the pcm arena changed"


STREAM_KW = dict(dsd_rate=1, output_rate=88200, channels=2, fmt="P", endianness="L", block_size=4096, filter="E", bit_depth=24, dither="T", seed=5)


@gpu
def test_whole_stream_twin_at_effort_1(engine_lib, oracle_mod):
    """d2d_convert_stream_flac_effort with chunks of 3072 frames: blocks straddle chunks, a remainder is carried, the last block is short"""
    d = engine_lib
    nbytes = 4096 * 10
    chans = [synth("sine", nbytes, seed=3), synth("sine", nbytes, seed=3, amp=0.3)]      # correlated channels: a stereo mode pays
    chunk = 3 * 4096
    pos = [0]

    def read(cap):
        a = pos[0]
        b = min(nbytes, a + cap)
        pos[0] = b
        return pack_layout([c[a:b] for c in chans], "P", 4096).tobytes() if b > a else b""

    ref, rf = oracle_mod.Oracle(**STREAM_KW).translate(pack_layout(chans, "P", 4096))
    want, res, _ = d.flac_encode_host(2, 24, ref[:rf * 6], first_block=0, final=True, effort=SEARCH)
    plain = d.flac_encode_host(2, 24, ref[:rf * 6], first_block=0, final=True)[0]
    out = []
    e = d.Engine(**STREAM_KW)
    stats = e.convert_stream_flac(read, out.append, total_bytes_per_channel=nbytes, chunk_bytes_per_channel=chunk, effort=SEARCH)
    e.close()
    assert len(out) > 2 and rf % 4096 and rf > 2 * 4096 and (chunk * 8 // 32) % 4096
    assert b"".join(out) == want and want != plain and len(want) <= len(plain)
    assert (stats.samples_per_channel, stats.blocks, stats.min_frame_bytes, stats.max_frame_bytes) == \
           (rf, rf // 4096 + 1, res.min_frame_bytes, res.max_frame_bytes)
    assert np.array_equal(S.decode(want, 2, 24)[0], R.unpack_pcm(ref[:rf * 6], 2, 24))


def _audio(flac):
    pos, last = 4, False
    while not last:
        last, blen = bool(flac[pos] & 0x80), int.from_bytes(flac[pos + 1:pos + 4], "big")
        pos += 4 + blen
    return flac[pos:]


@gpu
def test_cli_flac_effort_1_gpu_equals_the_host_sink_except_md5(engine_lib, tmp_path):
    if not os.path.exists(CLI):
        engine_lib.build_library()
    n = 4096 * 6 + 500
    chans = [synth("sine", n, seed=7), synth("sine", n, seed=7, amp=0.25)]
    for name in ("host", "gpu", "plain"):
        (tmp_path / name).mkdir()
        write_dsf(str(tmp_path / name / "y.dsf"), chans)
    args = [CLI, "convert", "-o", "f", "-r", "88200", "-b", "24", "-d", "T", "-q"]
    subprocess.check_call(args + ["--flac-effort", "1", str(tmp_path / "host" / "y.dsf")])
    subprocess.check_call(args + ["--flac-effort", "1", "--gpu-flac", str(tmp_path / "gpu" / "y.dsf")])
    subprocess.check_call(args + [str(tmp_path / "plain" / "y.dsf")])
    h, g, p = ((tmp_path / k / "y.flac").read_bytes() for k in ("host", "gpu", "plain"))
    assert len(h) == len(g) and h[:26] == g[:26] and h[42:] == g[42:]
    assert g[26:42] == bytes(16) and h[26:42] != bytes(16)          # STREAMINFO's MD5: "not computed" on the GPU path
    assert h[26:42] == p[26:42] and len(h) < len(p)                 # the same samples as the effort-0 file, in fewer bytes
    back, sizes, _ = S.decode(_audio(g), 2, 24)
    assert np.array_equal(back, R.decode(_audio(p), 2, 24)[0]) and back.shape[0] == n * 8 // 32
    si = g[8:42]
    assert int.from_bytes(si[4:7], "big") == min(sizes) and int.from_bytes(si[7:10], "big") == max(sizes)
    # an effort the encoders do not know is refused
    r = subprocess.run(args + ["--flac-effort", "2", str(tmp_path / "plain" / "y.dsf")], capture_output=True, text=True)
    assert r.returncode != 0 and "effort" in r.stderr
