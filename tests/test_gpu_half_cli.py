"""`dsd2dxd_amd_cli convert|levels -r 44100|48000` (Rdsd2Pcm::create_half and its siblings): synthesised stereo DSF files become CD-rate
WAV and FLAC files.  The WAV's header says 44100 and its data are the halved engine's own d2d_translate output; the host sink's FLAC files
and the --gpu-flac path's are equal in every byte at both rates and `verify` accepts them; `levels -r 44100` prints the halved engine's
peak; a two-track --album --replaygain at 48000 carries the album fields on both paths; what the halved engine refuses is refused with its
message before any device call."""
import os
import subprocess

import numpy as np
import pytest

from helpers import pack_layout, synth, write_dsf

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "dsd2dxd_amd", "dsd2dxd_amd_cli")
LENGTHS = (4096 * 6 + 300, 4096 * 4)                    # bytes per channel: 6219 and 4096 sums at 88.2 kHz -> 3110 and 2048 frames
KW = dict(dsd_rate=1, channels=2, fmt="P", endianness="L", block_size=4096, filter="E", seed=0)


def two(n, seed):
    return [synth("sine", n, seed=seed, freq=440.0), synth("pink", n, seed=seed + 1, amp=0.3)]


def tracks_in(tmp_path, name):
    (tmp_path / name).mkdir()
    paths, chans = [], []
    for k, n in enumerate(LENGTHS):
        chans.append(two(n, 10 * k + 1))
        paths.append(str(tmp_path / name / f"t{k}.dsf"))
        write_dsf(paths[-1], chans[-1])
    return paths, chans


def convert(paths, ext, *switches):
    r = subprocess.run([CLI, "convert", "-q"] + list(switches) + paths, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return [open(p[:-4] + ext, "rb").read() for p in paths]


def engine_bytes(d, chans, **kw):
    e = d.Engine.create_half(**dict(KW, **kw))
    try:
        want, frames = e.translate(pack_layout(chans, "P", 4096))
        return want.copy(), frames, e.peak_dbfs()
    finally:
        e.close()


def wav_chunks(data):
    assert data[:4] == b"RIFF" and data[8:12] == b"WAVE"
    pos, out = 12, {}
    while pos + 8 <= len(data):
        size = int.from_bytes(data[pos + 4:pos + 8], "little")
        out[data[pos:pos + 4]] = data[pos + 8:pos + 8 + size]
        pos += 8 + size + (size & 1)
    return out


@gpu
def test_wav_at_44100_holds_the_halved_engines_frames(engine_lib, tmp_path):
    d = engine_lib
    if not os.path.exists(CLI):
        d.build_library()
    paths, chans = tracks_in(tmp_path, "wav")
    files = convert(paths, ".wav", "-r", "44100", "-b", "16", "-o", "w")
    for k in range(2):
        ch = wav_chunks(files[k])
        fmt = ch[b"fmt "]
        assert int.from_bytes(fmt[2:4], "little") == 2 and int.from_bytes(fmt[4:8], "little") == 44100 and int.from_bytes(fmt[14:16], "little") == 16
        want, frames, _ = engine_bytes(d, chans[k], output_rate=44100, bit_depth=16, dither="T")
        assert frames == (LENGTHS[k] // 4 + 1) // 2
        assert np.array_equal(np.frombuffer(ch[b"data"], dtype=np.uint8), want), k
    # -a: the rate's suffix on the file name
    ap, _ = tracks_in(tmp_path, "append")
    r = subprocess.run([CLI, "convert", "-q", "-r", "44100", "-b", "16", "-o", "w", "-a", ap[0]], capture_output=True, text=True)
    assert r.returncode == 0 and os.path.exists(ap[0][:-4] + "_44_1K.wav"), (r.stderr, os.listdir(os.path.dirname(ap[0])))


@gpu
@pytest.mark.parametrize("rate", [44100, 48000])
def test_flac_on_both_paths_is_equal_in_every_byte(engine_lib, tmp_path, rate):
    from test_gpu_mix_cli import decoded, streaminfo
    d = engine_lib
    args = ["-r", str(rate), "-b", "24", "-d", "T", "-o", "f"]
    host_paths, chans = tracks_in(tmp_path, "host")
    host = convert(host_paths, ".flac", *args)
    gpu_files = convert(tracks_in(tmp_path, "gpu")[0], ".flac", *args, "--gpu-flac", "--flac-md5", "--flac-verify")
    for k in range(2):
        want, frames, _ = engine_bytes(d, chans[k], output_rate=rate, bit_depth=24, dither="T")
        assert streaminfo(host[k]) == (2, 24, frames)
        assert int.from_bytes(host[k][18:21], "big") >> 4 == rate                # STREAMINFO's sample rate
        assert gpu_files[k] == host[k], k
        assert np.array_equal(decoded(d, host[k], 2), want), k
    v = subprocess.run([CLI, "verify"] + [p[:-4] + ".flac" for p in host_paths], capture_output=True, text=True)
    assert v.returncode == 0 and [l.endswith(": ok") for l in v.stdout.splitlines()] == [True] * 2, (v.stdout, v.stderr)


@gpu
def test_levels_at_44100_reports_the_halved_engines_peak(engine_lib, tmp_path):
    d = engine_lib
    paths, chans = tracks_in(tmp_path, "levels")
    r = subprocess.run([CLI, "levels", "-r", "44100", paths[0]], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    _, _, want = engine_bytes(d, chans[0], output_rate=44100, bit_depth=32, dither="X")
    assert r.stdout.splitlines()[0] == "t0.dsf: %.4f dBFS" % want, (r.stdout, want)


@gpu
def test_album_with_replaygain_at_48000(engine_lib, tmp_path):
    from test_gpu_mix_cli import streaminfo
    args = ["-r", "48000", "-b", "24", "-d", "T", "-o", "f", "--album", "--replaygain"]
    host = convert(tracks_in(tmp_path, "album_host")[0], ".flac", *args)
    gpu_files = convert(tracks_in(tmp_path, "album_gpu")[0], ".flac", *args, "--gpu-flac", "--flac-md5")
    for k in range(2):
        assert gpu_files[k] == host[k], k
        assert streaminfo(host[k])[:2] == (2, 24) and int.from_bytes(host[k][18:21], "big") >> 4 == 48000
        for field in (b"REPLAYGAIN_TRACK_GAIN=", b"REPLAYGAIN_ALBUM_GAIN=", b"REPLAYGAIN_ALBUM_PEAK="):
            assert field in host[k][:4096], (k, field)


def test_refusals_name_their_reason(engine_lib, tmp_path):
    """(no GPU needed: every refusal comes before the first device call)"""
    d = engine_lib
    if not os.path.exists(CLI):
        d.build_library()
    ok = str(tmp_path / "ok.dsf")
    write_dsf(ok, two(4096, 3))
    base = [CLI, "convert", "-q", "-o", "w", "-b", "24"]
    for extra, frag in ((["-r", "44100", "-d", "N"], "noise-shaped"), (["-r", "48000", "-t", "D"], "dsd2pcm"), (["-r", "44100", "-t", "S"], "two-stage"),
                        (["-r", "44100", "--downmix", "mono"], "does not combine with a mix"), (["-r", "22050"], "Invalid output rate"),
                        (["-r", "44100", "--tap-bits", "32"], "32-bit taps")):
        r = subprocess.run(base + extra + [ok], capture_output=True, text=True)
        assert r.returncode == 1 and frag in r.stderr, (extra, r.stderr)
        assert "--tap-bits" in extra or not os.path.exists(ok[:-4] + ".wav"), extra          # (the tap grid is the run's to refuse: the sink is open by then)
    r = subprocess.run([CLI, "levels", "-r", "44100", "-t", "S", ok], capture_output=True, text=True)
    assert r.returncode == 1 and "two-stage" in r.stderr, r.stderr
