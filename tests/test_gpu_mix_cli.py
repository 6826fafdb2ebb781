"""`dsd2dxd_amd_cli convert|levels --downmix` (Rdsd2Pcm::set_downmix): synthesised 5.1 DSF files become stereo FLAC files.  The host
sink's files and the --gpu-flac path's are equal in every byte, alone and as an --album; the decoded PCM is the mixed engine's own
d2d_translate output; `verify` accepts the files; `levels --downmix stereo` prints the mixed engine's peak; a container whose layout no
preset serves is refused with a message; --mix takes decimal gains."""
import os
import subprocess

import numpy as np
import pytest

from helpers import pack_layout, random_bytes, synth, write_dsf

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "dsd2dxd_amd", "dsd2dxd_amd_cli")
ARGS = ["convert", "-o", "f", "-r", "88200", "-b", "24", "-d", "T", "-q"]
LENGTHS = (4096 * 5 + 300, 4096 * 4)                    # bytes per channel: 5195 and 4096 frames at 88.2 kHz (a partial last FLAC block, and exactly one)
KW = dict(dsd_rate=1, output_rate=88200, channels=6, fmt="P", endianness="L", block_size=4096, filter="E", bit_depth=24, dither="T", seed=0)


def six(n, seed):
    return [synth("sine", n, seed=seed, freq=440.0), synth("sine", n, seed=seed + 1, freq=660.0), synth("pink", n, seed=seed + 2, amp=0.3),
            synth("sine", n, seed=seed + 3, freq=50.0), random_bytes(n, seed + 4), synth("pink", n, seed=seed + 5, amp=0.2)]


def write_dsf_51(path, chans, channel_type=7):
    """helpers.write_dsf, with the fmt chunk's channel type set (7: 5.1, FL FR C LFE BL BR)"""
    write_dsf(path, chans)
    with open(path, "r+b") as f:
        f.seek(28 + 20)
        f.write(int(channel_type).to_bytes(4, "little"))


def tracks_in(tmp_path, name):
    (tmp_path / name).mkdir()
    paths, chans = [], []
    for k, n in enumerate(LENGTHS):
        chans.append(six(n, 10 * k + 1))
        paths.append(str(tmp_path / name / f"t{k}.dsf"))
        write_dsf_51(paths[-1], chans[-1])
    return paths, chans


def convert(paths, *switches):
    r = subprocess.run([CLI] + ARGS + list(switches) + paths, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return [open(p[:-4] + ".flac", "rb").read() for p in paths]


def streaminfo(data):
    assert data[:4] == b"fLaC" and data[4] & 0x7F == 0
    v = int.from_bytes(data[18:26], "big")
    return ((v >> 41) & 7) + 1, ((v >> 36) & 31) + 1, v & 0xFFFFFFFFF          # channels, depth, samples per channel


def decoded(d, data, channels):
    pos, last = 4, False
    while not last:
        last = bool(data[pos] & 0x80)
        pos += 4 + int.from_bytes(data[pos + 1:pos + 4], "big")
    total = streaminfo(data)[2]
    pcm, frames, check = d.flac_decode_host(channels, 24, np.frombuffer(data[pos:], dtype=np.uint8), capacity=(total + 4096) * 3 * channels)
    assert frames == total and check.bad_blocks == 0
    return np.frombuffer(bytes(pcm[:frames * 3 * channels]), dtype=np.uint8)


@gpu
def test_downmix_to_stereo_flac_on_both_paths_and_as_an_album(engine_lib, tmp_path):
    d = engine_lib
    if not os.path.exists(CLI):
        d.build_library()
    host_paths, chans = tracks_in(tmp_path, "host")
    host = convert(host_paths, "--downmix", "stereo")
    gpu_files = convert(tracks_in(tmp_path, "gpu")[0], "--downmix", "stereo", "--gpu-flac", "--flac-md5")
    album_host = convert(tracks_in(tmp_path, "album_host")[0], "--downmix", "stereo", "--album")
    album_gpu = convert(tracks_in(tmp_path, "album_gpu")[0], "--downmix", "stereo", "--album", "--gpu-flac", "--flac-md5", "--flac-verify")
    coef = d.mix_preset(6, 2, d.MIX_LAYOUT_5_1)
    for k in range(2):
        assert streaminfo(host[k])[:2] == (2, 24)
        assert gpu_files[k] == host[k] and album_host[k] == host[k] and album_gpu[k] == host[k], k
        e = d.Engine(mix=coef, **KW)
        want, frames = e.translate(pack_layout(chans[k], "P", 4096))
        e.close()
        assert frames == LENGTHS[k] // 4 == streaminfo(host[k])[2]
        assert np.array_equal(decoded(d, host[k], 2), want), k
    v = subprocess.run([CLI, "verify"] + [p[:-4] + ".flac" for p in host_paths], capture_output=True, text=True)
    assert v.returncode == 0 and [l.endswith(": ok") for l in v.stdout.splitlines()] == [True] * 2, (v.stdout, v.stderr)
    # mono, and an explicit matrix: the files are as wide as the matrix has rows
    mono = convert(tracks_in(tmp_path, "mono")[0][:1], "--downmix", "mono", "--gpu-flac")
    assert streaminfo(mono[0])[:2] == (1, 24)
    ms_paths, _ = tracks_in(tmp_path, "mix")
    ms = convert(ms_paths[:1], "--mix", "0.5,0.5,0,0,0,0; 0.5,-0.5,0,0,0,0; 0,0,1,0,0,0")
    assert streaminfo(ms[0])[:2] == (3, 24)
    e = d.Engine(mix=[[16384, 16384, 0, 0, 0, 0], [16384, -16384, 0, 0, 0, 0], [0, 0, 32768, 0, 0, 0]], **KW)
    want, _ = e.translate(pack_layout(chans[0], "P", 4096))
    e.close()
    assert np.array_equal(decoded(d, ms[0], 3), want)


@gpu
def test_levels_downmix_reports_the_folded_peak(engine_lib, tmp_path):
    d = engine_lib
    paths, chans = tracks_in(tmp_path, "levels")
    r = subprocess.run([CLI, "levels", "-r", "88200", "--downmix", "stereo", paths[0]], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    e = d.Engine(mix=d.mix_preset(6, 2), **dict(KW, bit_depth=32, dither="X"))
    e.translate(pack_layout(chans[0], "P", 4096))
    want = e.peak_dbfs()
    e.close()
    plain = subprocess.run([CLI, "levels", "-r", "88200", paths[0]], capture_output=True, text=True)
    assert r.stdout.splitlines()[0] == "t0.dsf: %.4f dBFS" % want, (r.stdout, want)
    assert plain.returncode == 0 and plain.stdout.splitlines()[0] != r.stdout.splitlines()[0]


def test_refusals_name_their_reason(engine_lib, tmp_path):
    """(no GPU needed: every refusal comes before the first device call)"""
    n = 4096
    odd = str(tmp_path / "odd.dsf")
    write_dsf_51(odd, six(n, 3), channel_type=1)                             # six channels that call themselves mono
    r = subprocess.run([CLI] + ARGS + ["--downmix", "stereo", odd], capture_output=True, text=True)
    assert r.returncode == 1 and "downmix" in r.stderr.lower() and not os.path.exists(odd[:-4] + ".flac"), r.stderr
    ok = str(tmp_path / "ok.dsf")
    write_dsf_51(ok, six(n, 3))
    for extra, code, frag in ((["--downmix", "quad"], 2, "stereo or mono"), (["--mix", "1,0;0"], 2, "same number"), (["--mix", "1,0"], 1, "one column per channel"),
                              (["--downmix", "stereo", "--mix", "1,0,0,0,0,0"], 2, "one of them"), (["--downmix", "stereo", "-d", "N"], 1, "noise-shaped"),
                              (["--downmix", "stereo", "--tap-bits", "32"], 1, "32-bit taps")):
        r = subprocess.run([CLI] + ARGS + extra + [ok], capture_output=True, text=True)
        assert r.returncode == code and frag in r.stderr, (extra, r.stderr)


@gpu
def test_dff_channel_ids_choose_the_preset(engine_lib, tmp_path):
    """four channels are quad or L R C LFE by their CHNL ids: `levels --downmix stereo` prints the peak of the engine mixed with that preset"""
    from test_mix_cpu import _dff
    d = engine_lib
    n = 4096 * 3
    chans = six(n, 40)[:4]
    lines = {}
    for name, ids, layout in (("quad", [b"SLFT", b"SRGT", b"LS  ", b"RS  "], d.MIX_LAYOUT_QUAD), ("lrclfe", [b"SLFT", b"SRGT", b"C   ", b"LFE "], d.MIX_LAYOUT_LRC_LFE)):
        path = str(tmp_path / (name + ".dff"))
        _dff(path, ids, nbytes=n)
        data = np.stack([c for c in chans], axis=1).reshape(-1).tobytes()          # the same audio behind both headers
        with open(path, "r+b") as f:
            f.seek(-len(data), os.SEEK_END)
            f.write(data)
        r = subprocess.run([CLI, "levels", "-r", "88200", "--downmix", "stereo", path], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        e = d.Engine(mix=d.mix_preset(4, 2, layout), **dict(KW, channels=4, fmt="I", endianness="M", bit_depth=32, dither="X"))
        e.translate(np.frombuffer(data, dtype=np.uint8))
        lines[name] = r.stdout.splitlines()[0]
        assert lines[name] == "%s.dff: %.4f dBFS" % (name, e.peak_dbfs()), (r.stdout, e.peak_dbfs())
        e.close()
    assert lines["quad"].split(": ")[1] != lines["lrclfe"].split(": ")[1]
