"""`dsd2dxd_amd_cli convert --album` (Rdsd2Pcm::convert_album): three small DSF files as one album.  The files equal the ones written
without --album outside the VORBIS_COMMENT block; with --replaygain the five fields are there in order, album gain and album peak are
the same text in all three files and are d2d_loud_finish_album / d2d_loud_true_peak_album of host-twin meters over the decoded PCM;
`verify` accepts every file; the --gpu-flac files and the host path's are equal in every byte."""
import os
import subprocess

import numpy as np
import pytest

from helpers import synth, write_dsf
from test_loudness_cpu import vorbis_fields

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "dsd2dxd_amd", "dsd2dxd_amd_cli")
NAMES = ("a", "b", "c")
LENGTHS = (4096 * 44 + 500, 4096 * 47, 4096 * 61 + 7)               # bytes per channel: 45181, 48128 and 62465 frames at 88.2 kHz, two or three 400 ms blocks each
AMPS = (0.35, 0.04, 0.2)                                             # the second track lies 19 dB under the first: under the relative gate
ARGS = ["convert", "-o", "f", "-r", "88200", "-b", "24", "-d", "T", "-q"]
EVERYTHING = ["--gpu-flac", "--replaygain", "--true-peak", "--flac-md5", "--flac-verify"]
FIELDS = ["REPLAYGAIN_REFERENCE_LOUDNESS", "REPLAYGAIN_TRACK_GAIN", "REPLAYGAIN_TRACK_PEAK", "REPLAYGAIN_ALBUM_GAIN", "REPLAYGAIN_ALBUM_PEAK"]


def album_dir(tmp_path, name, channels=2):
    """a folder with the three tracks; returns the DSF paths"""
    (tmp_path / name).mkdir()
    paths = []
    for k, n in enumerate(LENGTHS):
        chans = [synth("sine", n, seed=20 + k, amp=AMPS[k], freq=500.0 + 400 * k), synth("pink", n, seed=30 + k, amp=0.3 * AMPS[k])][:channels]
        paths.append(str(tmp_path / name / f"{NAMES[k]}.dsf"))
        write_dsf(paths[-1], chans)
    return paths


def convert(paths, *switches):
    r = subprocess.run([CLI] + ARGS + list(switches) + paths, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return [open(p[:-4] + ".flac", "rb").read() for p in paths]


def without_comment(data):
    """a FLAC file with its VORBIS_COMMENT block cut out (the `last` flags apart, which the block's place decides)"""
    assert data[:4] == b"fLaC"
    pos, last, out = 4, False, [data[:4]]
    while not last:
        last, kind = bool(data[pos] & 0x80), data[pos] & 0x7F
        size = int.from_bytes(data[pos + 1:pos + 4], "big")
        if kind != 4:
            out.append(bytes([kind]) + data[pos + 1:pos + 4 + size])
        pos += 4 + size
    return b"".join(out) + data[pos:]


def decoded(d, data):
    pos, last = 4, False
    while not last:
        last = bool(data[pos] & 0x80)
        pos += 4 + int.from_bytes(data[pos + 1:pos + 4], "big")
    total = int.from_bytes(data[18:26], "big") & 0xFFFFFFFFF              # STREAMINFO's samples per channel
    pcm, frames, check = d.flac_decode_host(2, 24, np.frombuffer(data[pos:], dtype=np.uint8), capacity=(total + 4096) * 6)
    assert frames == total
    assert check.bad_blocks == 0
    return np.frombuffer(bytes(pcm[:frames * 6]), dtype=np.uint8)


@gpu
def test_album_files_tags_and_both_paths(engine_lib, tmp_path):
    d = engine_lib
    if not os.path.exists(CLI):
        d.build_library()
    tracks = convert(album_dir(tmp_path, "tracks"), *EVERYTHING)
    paths = album_dir(tmp_path, "album")
    album = convert(paths, "--album", *EVERYTHING)
    host = convert(album_dir(tmp_path, "host"), "--album", "--replaygain", "--true-peak")
    meters = []
    for k in range(3):
        assert without_comment(album[k]) == without_comment(tracks[k]), f"track {k} differs outside the comment block"
        assert host[k] == album[k], f"track {k}: the host path's file is not the --gpu-flac path's"
        fields = vorbis_fields(paths[k][:-4] + ".flac")
        assert [f.split("=")[0] for f in fields] == FIELDS
        assert fields[:3] == vorbis_fields(str(tmp_path / "tracks" / f"{NAMES[k]}.flac"))
        pcm = decoded(d, album[k])
        m = d.LoudMeter(2, 88200, true_peak=True)
        cells, io = d.loud_measure_host(2, 24, 88200, pcm)
        partial = io.cells_out > io.subblocks * 2
        m.add(cells, has_partial=partial)
        m.add_true_peaks(d.true_peak_measure_host(2, 24, 88200, pcm)[0], has_partial=partial)
        meters.append((m, fields))
    r = d.loud_finish_album([m for m, _ in meters])
    want = ["REPLAYGAIN_ALBUM_GAIN=%+06.2f dB" % r.gain_db, "REPLAYGAIN_ALBUM_PEAK=%.6f" % d.loud_true_peak_album([m for m, _ in meters])]
    assert r.valid == 1 and r.blocks_gated > 0                             # the quiet track's blocks fall to the relative gate
    for k, (m, fields) in enumerate(meters):
        assert fields[3:] == want, (k, fields, want)
        assert fields[1] == "REPLAYGAIN_TRACK_GAIN=%+06.2f dB" % m.finish().gain_db and fields[2] == "REPLAYGAIN_TRACK_PEAK=%.6f" % m.true_peak()
    assert len({f[1] for _, f in meters}) == 3                             # ... and the track gains differ, so the album's is none of theirs by copy
    v = subprocess.run([CLI, "verify"] + [p[:-4] + ".flac" for p in paths], capture_output=True, text=True)
    assert v.returncode == 0 and [l.endswith(": ok") for l in v.stdout.splitlines()] == [True] * 3, (v.stdout, v.stderr)


@gpu
def test_album_without_replaygain_changes_no_byte(engine_lib, tmp_path):
    tracks = convert(album_dir(tmp_path, "tracks"), "--gpu-flac", "--flac-md5")
    album = convert(album_dir(tmp_path, "album"), "--album", "--gpu-flac", "--flac-md5")
    host = convert(album_dir(tmp_path, "host"), "--album")
    assert album == tracks and host == tracks and b"REPLAYGAIN" not in album[0]


@gpu
def test_a_track_of_another_channel_count_is_named(engine_lib, tmp_path):
    paths = album_dir(tmp_path, "mixed")
    write_dsf(paths[1], [synth("sine", LENGTHS[1], seed=5)])               # b.dsf becomes mono
    r = subprocess.run([CLI] + ARGS + ["--album", "--gpu-flac"] + paths, capture_output=True, text=True)
    assert r.returncode == 1 and "b.dsf" in r.stderr and "channel count" in r.stderr, r.stderr
    r = subprocess.run([CLI] + ARGS[:2] + ["w"] + ARGS[3:] + ["--album"] + paths, capture_output=True, text=True)
    assert r.returncode == 2 and "--album" in r.stderr                     # an album is FLAC files
