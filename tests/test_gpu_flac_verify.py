"""d2d_flac_verify_device (include/dsd2dxd_amd.h, "Verifying the frames"): the frames an encode call packed are parsed, decoded and
compared with their PCM on the GPU, at every effort, and the record equals d2d_flac_verify_host's on the downloaded bytes -- the same
parser (csrc/flac/flac_parse.h) compiled for the host, which tests/test_flac_verify_cpu.py pins and runs sanitised on damaged frames.
Detection runs that file's crafted frames, one per reason, and nothing else damaged.  Then: what a call touches, the verified
whole-stream driver and the CLI's --flac-verify.  No file exceeds three blocks but the two (19 and 9 blocks) that spread one file's
frames over several workgroups of the status kernel."""
import os
import subprocess

import numpy as np
import pytest

import flac_ref as R
from helpers import pack_layout, synth, write_dsf
from test_flac_lpc_cpu import CASES as LPC_CASES
from test_flac_verify_cpu import (BAD_CRC16, BAD_NONE, BAD_SAMPLES, BAD_SIZE, BLOCK, CRAFT_CH, CRAFT_DEPTH, CRAFT_FIRST, EFFORTS, LENGTHS, MUTATIONS, NONE,
                                  clean, craft_stream, damaged, make_signal, mutations, nblocks)
from test_gpu_containment import Arena, describe, fill_bytes, violations
from test_gpu_flac_search import STREAM_KW, _dev, _host

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "dsd2dxd_amd", "dsd2dxd_amd_cli")
CHECK_BYTES = 24


def records(t, n):
    """n d2d_flac_check records of a downloaded uint8 array as tuples"""
    out = []
    for i in range(n):
        r = t[CHECK_BYTES * i:CHECK_BYTES * (i + 1)]
        out.append((int(r[:8].view(np.uint64)[0]),) + tuple(int(v) for v in r[8:].view(np.uint32)))
    return out


class Batch:
    """files [(pcm uint8 array, first_block, final)] in device buffers of their own, one workspace, result and check records"""

    def __init__(self, d, channels, depth, files):
        self.d, self.ch, self.depth, self.files = d, channels, depth, files
        fb = channels * (2 if depth == 16 else 3)
        n = len(files)
        self.ios = (d.FlacIO * n)()
        self.pcm, self.out, self.ws_at, self.ws_bytes = [], [], [], 0
        self.rec = _dev(np.full(16 * n, 0xEE, dtype=np.uint8))
        self.chk = _dev(np.full(CHECK_BYTES * n, 0xDD, dtype=np.uint8))
        for i, (pcm, first, final) in enumerate(files):
            frames = pcm.size // fb
            cap = d.flac_bound_bytes(channels, depth, frames, final)
            tp, to = _dev(pcm if pcm.size else np.zeros(16, dtype=np.uint8)), _dev(np.full(max(cap, 16), 0xA5, dtype=np.uint8))
            self.pcm.append(tp)
            self.out.append(to)
            io = self.ios[i]
            io.pcm, io.frames, io.first_block, io.final = tp.data_ptr(), frames, first, int(final)
            io.out, io.out_capacity_bytes, io.result = to.data_ptr(), cap, self.rec.data_ptr() + 16 * i
            self.ws_at.append(self.ws_bytes)
            self.ws_bytes += d.flac_workspace_bytes(channels, depth, frames, final)
        self.ws = _dev(np.zeros(max(self.ws_bytes, 16), dtype=np.uint8))

    def encode(self, effort, stream=None):
        self.d.flac_encode_device(self.ch, self.depth, self.ios, self.ws.data_ptr(), self.ws_bytes, stream=stream, effort=effort)

    def verify(self, stream=None):
        self.d.flac_verify_device(self.ch, self.depth, self.ios, self.ws.data_ptr(), self.ws_bytes, self.chk.data_ptr(), stream=stream)

    def checks(self):
        return records(_host(self.chk), len(self.files))

    def frames(self, i):
        """(the packed bytes of file i, its size table) as the encode call left them"""
        bytes_out = int(_host(self.rec).view(np.uint64)[2 * i])
        blocks = self.ios[i].blocks
        sizes = _host(self.ws)[self.ws_at[i]:self.ws_at[i] + 4 * blocks].view(np.uint32).copy()
        return _host(self.out[i])[:bytes_out].copy(), sizes

    def host_checks(self):
        out = []
        for i, (pcm, first, final) in enumerate(self.files):
            b, sizes = self.frames(i)
            out.append(self.d.flac_verify_host(self.ch, self.depth, pcm, b, first_block=first, final=final, sizes=sizes).as_tuple())
        return out


@gpu
@pytest.mark.parametrize("depth", (16, 20, 24))
@pytest.mark.parametrize("channels", (1, 2, 3, 8))
@pytest.mark.parametrize("effort", EFFORTS)
def test_clean_verify_of_the_host_cases(engine_lib, effort, channels, depth):
    """the round-trip shapes of the CPU test, the ten lengths of one (channels, depth) in one call"""
    sigs = [make_signal((i + channels + depth) % 5, n, channels, depth, 7 * i + channels) for i, n in enumerate(LENGTHS)]
    b = Batch(engine_lib, channels, depth, [(R.pack_pcm(x, depth), 126 + i, True) for i, x in enumerate(sigs)])
    b.encode(effort)
    b.verify()
    got = b.checks()
    assert got == [clean(n, nblocks(n)) for n in LENGTHS], got
    assert got == b.host_checks()
    # the frames are those of the host encoder: the verify pass read what the tests of the encoders compare
    for i, (pcm, first, final) in enumerate(b.files):
        assert b.frames(i)[0].tobytes() == engine_lib.flac_encode_host(channels, depth, pcm, first_block=first, final=final, effort=effort)[0]


@gpu
@pytest.mark.parametrize("effort", EFFORTS)
def test_clean_verify_of_the_lpc_cases(engine_lib, effort):
    for channels, depth in sorted({(c["samples"].shape[1], c["depth"]) for c in LPC_CASES}):
        mine = [c for c in LPC_CASES if (c["samples"].shape[1], c["depth"]) == (channels, depth)]
        b = Batch(engine_lib, channels, depth, [(R.pack_pcm(c["samples"], depth), c["first_block"], c["final"]) for c in mine])
        b.encode(effort)
        b.verify()
        got = b.checks()
        for c, g, io in zip(mine, got, b.ios):
            assert g == clean(io.frames_consumed, io.blocks), (c["name"], g)
        assert got == b.host_checks()


@gpu
@pytest.mark.parametrize("effort", EFFORTS)
def test_ragged_batches_back_to_back_on_a_callers_stream(engine_lib, effort):
    """three files, one empty and one with a last block of 100 samples; seventeen one-block files, one more than a pair of launches
    carries; one file of 19 blocks and a short one beside a file of 9, so that a file's frames spread over several workgroups of the
    status kernel (eight frames each) and the offsets of the later ones come from the sizes in front; encode and verify enqueued on a
    non-blocking stream with no synchronisation between them"""
    import torch
    ragged = [(2 * BLOCK + 100, True, 5), (0, True, 0), (BLOCK + 1000, False, 0x7FF)]
    many = [(BLOCK if i % 3 else 1000 + i, True, 120 + i) for i in range(17)]
    long = [(19 * BLOCK + 100, True, 0x7FE), (9 * BLOCK, True, 0)]
    for shapes in (ragged, long, many):
        sigs = [make_signal(i % 5, n, 2, 24, i) if n else np.zeros((0, 2), dtype=np.int64) for i, (n, _, _) in enumerate(shapes)]
        b = Batch(engine_lib, 2, 24, [(R.pack_pcm(x, 24), first, final) for x, (_, final, first) in zip(sigs, shapes)])
        torch.cuda.synchronize()
        s = torch.cuda.Stream()
        b.encode(effort, stream=s.cuda_stream)
        b.verify(stream=s.cuda_stream)
        s.synchronize()
        got = b.checks()
        want = [clean(n if final else n // BLOCK * BLOCK, nblocks(n) if final else n // BLOCK) for n, final, _ in shapes]
        assert got == want, got
        assert got == b.host_checks()
    assert want[0] == clean(1000, 1) and len(want) == 17


# ---- detection: the crafted cases of the CPU test, one per reason, and only those -------------------------------------------------------

@pytest.fixture(scope="module")
def crafted(engine_lib):
    x, pcm, frames, sizes = craft_stream(engine_lib)
    a, b = sizes[0], sizes[0] + sizes[1]
    return dict(x=x, pcm=pcm, frames=frames, sizes=sizes, muts=mutations(frames[a:b])[0])


def crafted_batch(d, c):
    """the crafted stream between two plain files, encoded on the device at effort 0: its bytes are those of the CPU test"""
    other = R.pack_pcm(make_signal(0, BLOCK + 5, CRAFT_CH, CRAFT_DEPTH, 1), CRAFT_DEPTH)
    b = Batch(d, CRAFT_CH, CRAFT_DEPTH, [(other, 0, True), (c["pcm"], CRAFT_FIRST, True), (other, 9, True)])
    b.encode(0)
    out, sizes = b.frames(1)
    assert out.tobytes() == c["frames"] and list(sizes) == c["sizes"]
    return b


@gpu
@pytest.mark.parametrize("name", MUTATIONS)
def test_detection_of_one_crafted_frame_per_reason(engine_lib, crafted, name):
    import torch
    d, c = engine_lib, crafted
    b = crafted_batch(d, c)
    out = np.frombuffer(damaged(c, name), dtype=np.uint8)
    b.out[1][:out.size] = torch.from_numpy(out.copy()).cuda()                # the same mutation, uploaded over the encoder's bytes
    b.verify()
    got = b.checks()
    want = d.flac_verify_host(CRAFT_CH, CRAFT_DEPTH, c["pcm"], out, first_block=CRAFT_FIRST, sizes=c["sizes"]).as_tuple()
    reason = c["muts"][name][1]
    assert got[1] == want and want[:4] == (c["x"].shape[0] - BLOCK, 3, 1, 1) and want[4] in (reason if isinstance(reason, tuple) else (reason,)), (got[1], want)
    assert got[0] == clean(BLOCK + 5, 2) and got[2] == clean(BLOCK + 5, 2)   # the neighbouring files, as the neighbouring blocks, are good


@gpu
def test_detection_of_a_wrong_size_entry_and_of_changed_pcm(engine_lib, crafted):
    import torch
    d, c = engine_lib, crafted
    # an entry of the size table: the one thing the verify call takes from the encoder
    for wrong, want in ((0, (BLOCK, 3, 2, 1, BAD_SIZE)), (c["sizes"][1] - 1, (BLOCK, 3, 2, 1, BAD_CRC16))):
        b = crafted_batch(d, c)
        sizes = list(c["sizes"])
        sizes[1] = wrong
        b.ws[b.ws_at[1]:b.ws_at[1] + 12] = torch.from_numpy(np.array(sizes, dtype=np.uint32).view(np.uint8).copy()).cuda()
        b.verify()
        got = b.checks()
        assert got[1] == want == d.flac_verify_host(CRAFT_CH, CRAFT_DEPTH, c["pcm"], c["frames"], first_block=CRAFT_FIRST, sizes=sizes).as_tuple(), got[1]
        assert got[0] == clean(BLOCK + 5, 2) and got[2] == clean(BLOCK + 5, 2)
    # untouched frames, one changed PCM sample: SAMPLES at its block only
    for frame_index, channel in ((BLOCK + 17, 1), (2 * BLOCK + 99, 0)):
        b = crafted_batch(d, c)
        at = (frame_index * CRAFT_CH + channel) * 3
        b.pcm[1][at] ^= 1
        b.verify()
        block = frame_index // BLOCK
        assert b.checks()[1] == (c["x"].shape[0] - (BLOCK, BLOCK, 100)[block], 3, 1, block, BAD_SAMPLES)


# ---- what a call touches --------------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("complement", (False, True))
def test_a_verify_call_writes_only_its_records_and_the_workspace(engine_lib, complement):
    """pcm, out, workspace, result records and check records each in an arena between guards, two complementary fills.  After a verify,
    out, pcm and the result records are byte for byte what the encode call left, nothing outside the workspace and the check records
    changed; a refused call changed nothing at all"""
    d, ch, depth = engine_lib, 2, 24
    shapes = ((BLOCK + 1000, True, 3), (0, True, 0), (2 * BLOCK + 100, False, 0x7FF), (17, True, 0))
    pcms = [R.pack_pcm(make_signal(i % 5, n, ch, depth, i) if n else np.zeros((0, 2), dtype=np.int64), depth) for i, (n, _, _) in enumerate(shapes)]
    caps = [d.flac_bound_bytes(ch, depth, n, f) for n, f, _ in shapes]
    wss = sum(d.flac_workspace_bytes(ch, depth, n, f) for n, f, _ in shapes)
    a_in, a_out, a_ws, a_rec, a_chk = Arena([p.size for p in pcms]), Arena(caps), Arena([wss]), Arena([16 * len(shapes)]), Arena([CHECK_BYTES * len(shapes)])
    arenas = (a_in, a_out, a_ws, a_rec, a_chk)
    fills = [fill_bytes(a.total, complement).copy() for a in arenas]
    for s, p in zip(a_in.starts, pcms):
        fills[0][s:s + p.size] = p
    t_in, t_out, t_ws, t_rec, t_chk = (_dev(f) for f in fills)
    tensors = (t_in, t_out, t_ws, t_rec, t_chk)
    ios = (d.FlacIO * len(shapes))()
    for i, (n, final, first) in enumerate(shapes):
        ios[i].pcm, ios[i].frames, ios[i].first_block, ios[i].final = t_in.data_ptr() + a_in.starts[i], n, first, int(final)
        ios[i].out, ios[i].out_capacity_bytes = t_out.data_ptr() + a_out.starts[i], caps[i]
        ios[i].result = t_rec.data_ptr() + a_rec.starts[0] + 16 * i
    ws_ptr, chk_ptr = t_ws.data_ptr() + a_ws.starts[0], t_chk.data_ptr() + a_chk.starts[0]
    d.flac_encode_device(ch, depth, ios, ws_ptr, wss, effort=12)
    before = [_host(t).copy() for t in tensors]

    def unchanged(what):
        for t, f, name in zip(tensors, before, ("pcm", "out", "workspace", "result records", "check records")):
            assert np.array_equal(_host(t), f), f"{what}: the {name} arena changed"

    for bad, code in ((dict(depth=12), -1), (dict(ch=9), -1), (dict(wss=wss - 1), -20), (dict(chk=chk_ptr + 4), -1), (dict(ws=ws_ptr + 8), -1), (dict(chk=0), -1)):
        with pytest.raises(d.D2DError) as ei:
            d.flac_verify_device(bad.get("ch", ch), bad.get("depth", depth), ios, bad.get("ws", ws_ptr), bad.get("wss", wss), bad.get("chk", chk_ptr))
        assert ei.value.code == code, bad
        unchanged(f"refused call {bad}")

    d.flac_verify_device(ch, depth, ios, ws_ptr, wss, chk_ptr)
    after = [_host(t) for t in tensors]
    for k, name in ((0, "pcm"), (1, "out"), (3, "result records")):
        assert np.array_equal(after[k], before[k]), f"the {name} arena changed"
    v = violations(a_ws, after[2], fills[2], [after[2][a_ws.starts[0]:a_ws.end(0)]])       # the inside is the call's own
    assert not v, "workspace: " + describe(v)
    want = np.zeros(len(shapes) * CHECK_BYTES, dtype=np.uint8)
    for i, (n, final, _) in enumerate(shapes):
        used = n if final else n // BLOCK * BLOCK
        want[CHECK_BYTES * i:CHECK_BYTES * i + 8] = np.array([used], dtype=np.uint64).view(np.uint8)
        want[CHECK_BYTES * i + 8:CHECK_BYTES * (i + 1)] = np.array([nblocks(used), 0, NONE, BAD_NONE], dtype=np.uint32).view(np.uint8)
    v = violations(a_chk, after[4], fills[4], [want])
    assert not v, "check records: " + describe(v)
    # the size table in front of each file's workspace is still the encoder's: a second verify gives the same records
    d.flac_verify_device(ch, depth, ios, ws_ptr, wss, chk_ptr)
    assert np.array_equal(_host(t_chk), after[4])


# ---- the whole-stream driver and the CLI ----------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("effort", EFFORTS)
def test_verified_stream_hands_write_the_same_bytes(engine_lib, effort):
    d = engine_lib
    nbytes = 4096 * 10
    chans = [synth("sine", nbytes, seed=3), synth("sine", nbytes, seed=3, amp=0.3)]
    chunk = 3 * 4096

    def run(verify):
        pos, out = [0], []

        def read(cap):
            a = pos[0]
            b = min(nbytes, a + cap)
            pos[0] = b
            return pack_layout([c[a:b] for c in chans], "P", 4096).tobytes() if b > a else b""

        e = d.Engine(**STREAM_KW)
        r = e.convert_stream_flac(read, out.append, total_bytes_per_channel=nbytes, chunk_bytes_per_channel=chunk, effort=effort, verify=verify)
        e.close()
        return out, r

    plain, stats = run(False)
    checked, (vstats, chk) = run(True)
    assert checked == plain and len(plain) > 2
    assert (vstats.samples_per_channel, vstats.blocks, vstats.min_frame_bytes, vstats.max_frame_bytes) == \
           (stats.samples_per_channel, stats.blocks, stats.min_frame_bytes, stats.max_frame_bytes)
    assert chk.as_tuple() == clean(stats.samples_per_channel, stats.blocks) and stats.blocks == 3 and stats.samples_per_channel % 4096


@gpu
def test_cli_flac_verify(engine_lib, tmp_path):
    if not os.path.exists(CLI):
        engine_lib.build_library()
    n = 4096 * 6 + 500
    chans = [synth("sine", n, seed=7), synth("sine", n, seed=7, amp=0.25)]
    for name in ("plain", "verified", "host"):
        (tmp_path / name).mkdir()
        write_dsf(str(tmp_path / name / "y.dsf"), chans)
    args = [CLI, "convert", "-o", "f", "-r", "88200", "-b", "24", "-d", "T", "-q", "--flac-effort", "12"]
    subprocess.check_call(args + ["--gpu-flac", str(tmp_path / "plain" / "y.dsf")])
    subprocess.check_call(args + ["--gpu-flac", "--flac-verify", str(tmp_path / "verified" / "y.dsf")])
    subprocess.check_call(args + [str(tmp_path / "host" / "y.dsf")])
    p, v = ((tmp_path / k / "y.flac").read_bytes() for k in ("plain", "verified"))
    assert v == p and v[26:42] == bytes(16)
    r = subprocess.run([CLI, "verify", str(tmp_path / "verified" / "y.flac"), str(tmp_path / "host" / "y.flac")], capture_output=True, text=True)
    lines = r.stdout.splitlines()
    assert r.returncode == 0 and lines[0].endswith(": ok (no MD5 in STREAMINFO)") and lines[1].endswith(": ok"), (r.stdout, r.stderr)
    for extra in (["--flac-verify"], ["--flac-verify", "-o", "w", "--gpu-flac"]):
        r = subprocess.run(args + extra + [str(tmp_path / "host" / "y.dsf")], capture_output=True, text=True)
        assert r.returncode != 0 and "--gpu-flac" in r.stderr, r.stderr
