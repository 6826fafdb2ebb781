"""FLAC effort 12 on the GPU (include/dsd2dxd_amd.h, "EFFORTS"): d2d_flac_encode_device_effort, d2d_convert_stream_flac_effort and the
CLI's --flac-effort 12 against d2d_flac_encode_host_effort -- the sink's own encoder, pinned to the definition by
tests/test_flac_lpc_cpu.py -- byte for byte.  The inputs are that file's CASES, so its assertion that they force every LPC order, the
fixed plan beside LPC candidates, silence, the clamped shift, every stereo assignment with an LPC subframe and the 25-bit LPC side
subframe covers what runs here; the cases of one (channels, depth) go through one call.  No file exceeds three blocks."""
import os
import subprocess

import numpy as np
import pytest

import flac_lpc_ref as P
import flac_ref as R
import flac_search_ref as S
from helpers import pack_layout, synth, write_dsf
from test_flac_lpc_cpu import CASES, ar, lpc_stereo
from test_gpu_containment import Arena, describe, fill_bytes, violations
from test_gpu_flac_search import STREAM_KW, _audio, _dev, _host, device_encode, host_encode

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "dsd2dxd_amd", "dsd2dxd_amd_cli")
LPC = 12

GROUPS = sorted({(c["samples"].shape[1], c["depth"]) for c in CASES})


@gpu
@pytest.mark.parametrize("channels,depth", GROUPS, ids=lambda v: str(v))
def test_the_cpu_cases_equal_the_host_encoder(engine_lib, channels, depth):
    mine = [c for c in CASES if (c["samples"].shape[1], c["depth"]) == (channels, depth)]
    files = [(R.pack_pcm(c["samples"], depth), c["first_block"], c["final"]) for c in mine]
    want = host_encode(engine_lib, channels, depth, files, effort=LPC)
    got = device_encode(engine_lib, channels, depth, files, effort=LPC)
    for c, g, w in zip(mine, got, want):
        assert g[1] == w[1], c["name"]                              # the result record
        assert g[0] == w[0], c["name"]                              # the frames
        assert g[2] == w[2], c["name"]                              # frames_consumed


def test_the_groups_reach_every_channel_count_depth_and_length():
    assert {ch for ch, _ in GROUPS} == {1, 2, 3, 8} and {d for _, d in GROUPS} == {16, 20, 24}
    assert {63, 64, 65, 1000, 4095, 4096} <= {c["samples"].shape[0] for c in CASES}
    assert max(c["samples"].shape[0] for c in CASES) <= 3 * 4096


# (frames, final, first_block)
RAGGED = [(0, False, 9), (63, True, 0), (64, True, 0x7F), (1000, True, 3), (4096, False, 0x7FF), (2 * 4096 + 17, True, 1000), (4096 + 2048, True, 77),
          (1000, False, 0), (4096 + 2048, False, 5)]


@gpu
def test_ragged_batch_and_determinism(engine_lib):
    sigs = [lpc_stereo(n, 24, S.MODES[i % 4], 40 + i) if n else np.zeros((0, 2), dtype=np.int64) for i, (n, _, _) in enumerate(RAGGED)]
    files = [(R.pack_pcm(s, 24), first, final) for s, (_, final, first) in zip(sigs, RAGGED)]
    want = host_encode(engine_lib, 2, 24, files, effort=LPC)
    got = device_encode(engine_lib, 2, 24, files, effort=LPC)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (i, RAGGED[i])
    assert got[0][1] == (0, 0, 0) and got[7][1] == (0, 0, 0)
    # LPC subframes were written: shorter than effort 1 where a whole block is there
    one = host_encode(engine_lib, 2, 24, files, effort=1)
    assert all(g[1][0] <= o[1][0] for g, o in zip(got, one)) and got[5][1][0] < one[5][1][0]
    assert device_encode(engine_lib, 2, 24, files, effort=LPC) == got          # the same call again: the same bytes


@gpu
def test_efforts_0_and_1_through_the_same_entry_are_the_old_kernels(engine_lib):
    files = [(R.pack_pcm(ar(4096 + 100, 2, 24, 6, 3), 24), 0, True)]
    for effort in (0, 1):
        assert device_encode(engine_lib, 2, 24, files, effort=effort) == host_encode(engine_lib, 2, 24, files, effort=effort)


@gpu
@pytest.mark.parametrize("complement", (False, True))
def test_a_call_writes_only_what_it_reports(engine_lib, complement):
    """as tests/test_gpu_flac_search.py at effort 1: out buffers back to back with exact capacities, the workspace and the result
    records between guards, two complementary fills.  After a successful effort-12 call only [0, bytes_out) of each out, the records
    and the inside of the workspace differ from the fill; after a refused call -- an unknown effort, a capacity a byte short --
    nothing does"""
    d, ch, depth = engine_lib, 2, 24
    shapes = ((4096 + 1000, True, 3), (0, True, 0), (2 * 4096 + 100, False, 0x7FF), (1024, True, 1), (64, True, 0))
    pcms = [R.pack_pcm(lpc_stereo(n, depth, S.MODES[(i + 1) % 4], i) if n else np.zeros((0, 2), dtype=np.int64), depth) for i, (n, _, _) in enumerate(shapes)]
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
        d.flac_encode_device(ch, depth, ios(), t_ws.data_ptr() + a_ws.starts[0], wss, effort=13)
    assert ei.value.code == -1 and "effort" in ei.value.message
    unchanged("unknown effort")
    with pytest.raises(d.D2DError) as ei:
        d.flac_encode_device(ch, depth, ios(short=2), t_ws.data_ptr() + a_ws.starts[0], wss, effort=LPC)
    assert ei.value.code == -20
    unchanged("capacity one byte short")

    want = host_encode(d, ch, depth, [(p, first, final) for p, (_, final, first) in zip(pcms, shapes)], effort=LPC)
    d.flac_encode_device(ch, depth, ios(), t_ws.data_ptr() + a_ws.starts[0], wss, effort=LPC)
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


@gpu
def test_whole_stream_twin_at_effort_12(engine_lib, oracle_mod):
    """d2d_convert_stream_flac_effort with chunks of 3072 frames: blocks straddle chunks, a remainder is carried, the last block is short"""
    d = engine_lib
    nbytes = 4096 * 10
    chans = [synth("sine", nbytes, seed=3), synth("pink", nbytes, seed=4, amp=0.098)]
    chunk = 3 * 4096
    pos = [0]

    def read(cap):
        a = pos[0]
        b = min(nbytes, a + cap)
        pos[0] = b
        return pack_layout([c[a:b] for c in chans], "P", 4096).tobytes() if b > a else b""

    ref, rf = oracle_mod.Oracle(**STREAM_KW).translate(pack_layout(chans, "P", 4096))
    want, res, _ = d.flac_encode_host(2, 24, ref[:rf * 6], first_block=0, final=True, effort=LPC)
    one = d.flac_encode_host(2, 24, ref[:rf * 6], first_block=0, final=True, effort=1)[0]
    out = []
    e = d.Engine(**STREAM_KW)
    stats = e.convert_stream_flac(read, out.append, total_bytes_per_channel=nbytes, chunk_bytes_per_channel=chunk, effort=LPC)
    e.close()
    assert len(out) > 2 and rf % 4096 and rf > 2 * 4096 and (chunk * 8 // 32) % 4096
    assert b"".join(out) == want and len(want) < len(one)
    assert (stats.samples_per_channel, stats.blocks, stats.min_frame_bytes, stats.max_frame_bytes) == \
           (rf, rf // 4096 + 1, res.min_frame_bytes, res.max_frame_bytes)
    back, _, infos = P.decode(want, 2, 24)
    assert np.array_equal(back, R.unpack_pcm(ref[:rf * 6], 2, 24))
    assert any(kind == "lpc" for _, subs in infos for kind, _, _ in subs)


@gpu
def test_cli_flac_effort_12_gpu_equals_the_host_sink_except_md5(engine_lib, tmp_path):
    if not os.path.exists(CLI):
        engine_lib.build_library()
    n = 4096 * 6 + 500
    chans = [synth("sine", n, seed=7), synth("pink", n, seed=8, amp=0.098)]
    for name in ("host", "gpu", "one"):
        (tmp_path / name).mkdir()
        write_dsf(str(tmp_path / name / "y.dsf"), chans)
    args = [CLI, "convert", "-o", "f", "-r", "88200", "-b", "24", "-d", "T", "-q"]
    subprocess.check_call(args + ["--flac-effort", "12", str(tmp_path / "host" / "y.dsf")])
    subprocess.check_call(args + ["--flac-effort", "12", "--gpu-flac", str(tmp_path / "gpu" / "y.dsf")])
    subprocess.check_call(args + ["--flac-effort", "1", str(tmp_path / "one" / "y.dsf")])
    h, g, p = ((tmp_path / k / "y.flac").read_bytes() for k in ("host", "gpu", "one"))
    assert len(h) == len(g) and h[:26] == g[:26] and h[42:] == g[42:]
    assert g[26:42] == bytes(16) and h[26:42] != bytes(16)          # STREAMINFO's MD5: "not computed" on the GPU path
    assert h[26:42] == p[26:42] and len(h) < len(p)                 # the same samples as the effort-1 file, in fewer bytes
    back, sizes, infos = P.decode(_audio(g), 2, 24)
    assert np.array_equal(back, P.decode(_audio(p), 2, 24)[0]) and back.shape[0] == n * 8 // 32
    assert any(kind == "lpc" for _, subs in infos for kind, _, _ in subs)
    si = g[8:42]
    assert int.from_bytes(si[4:7], "big") == min(sizes) and int.from_bytes(si[7:10], "big") == max(sizes)
    r = subprocess.run(args + ["--flac-effort", "13", str(tmp_path / "one" / "y.dsf")], capture_output=True, text=True)
    assert r.returncode != 0 and "effort" in r.stderr
