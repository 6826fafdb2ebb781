"""d2d_segments_move_host and d2d_segments_pack_host (include/dsd2dxd_amd.h, "A chunk's bookkeeping in one launch"): the CPU twins of
the segment calls, through the cases tests/test_gpu_segments.py runs on the device (tests/segments_cases.py); and tools/segments_fuzz.cpp,
the stand-alone program that runs the twins and their checks under the address and undefined-behaviour sanitisers."""
import ctypes as C
import os
import subprocess

import pytest

import segments_cases as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dsd2dxd_amd", "csrc")


def test_structures_have_the_public_layout(engine_lib):
    d = engine_lib
    assert C.sizeof(d.Segment) == 24 and C.sizeof(d.PackSrc) == 24
    assert C.sizeof(d.StreamIO) == 112 and C.sizeof(d.StreamsOptions) == 64
    assert d.StreamIO.stats.offset == 48 and d.StreamIO.check.offset == 72 and d.StreamIO.md5.offset == 96


@pytest.mark.parametrize("fill", S.FILLS)
def test_move_writes_the_ranges_and_nothing_else(engine_lib, fill):
    mem = S.HostMemory()
    S.check_move(engine_lib, engine_lib.segments_move_host, mem, mem, fill)


def test_move_refuses_overlap_and_changes_nothing(engine_lib):
    S.check_move_refusals(engine_lib, engine_lib.segments_move_host, S.HostMemory())


@pytest.mark.parametrize("fill", S.FILLS)
@pytest.mark.parametrize("case", ["few", "many"])
def test_pack_lays_the_segments_back_to_back(engine_lib, case, fill):
    mem = S.HostMemory()
    S.check_pack(engine_lib, engine_lib.segments_pack_host, mem, mem, case, fill)


@pytest.mark.parametrize("case,too_long", [("few", 2), ("few", 0), ("many", 5), ("many", 299)])
def test_pack_with_a_length_above_its_maximum_writes_only_the_table(engine_lib, case, too_long):
    mem = S.HostMemory()
    S.check_pack(engine_lib, engine_lib.segments_pack_host, mem, mem, case, S.FILLS[0], too_long=too_long)


def test_pack_of_nothing_and_refusals(engine_lib):
    S.check_pack_empty_and_refusals(engine_lib, engine_lib.segments_pack_host, S.HostMemory())


def test_twins_and_checks_sanitised(tmp_path):
    """tools/segments_fuzz.cpp: random segment lists against a bytewise model, the overlap check against the quadratic definition, the
    offsets arithmetic -- g++ alone, -fsanitize=address,undefined"""
    exe = str(tmp_path / "segments_fuzz")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(ROOT, "tools", "segments_fuzz.cpp"), os.path.join(CSRC, "batch", "d2d_segments_host.cpp"),
                    os.path.join(CSRC, "flac", "d2d_flac_host.cpp")], check=True)
    out = subprocess.run([exe, "400"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ok" in out.stdout
