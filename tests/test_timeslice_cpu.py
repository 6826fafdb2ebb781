"""shard_time (dsd2dxd_amd/shard.py): how ONE stream is cut along time for N ranks -- slices that tile the stream in order,
aligned begins, a halo of at least the preroll in front of every slice.  No GPU."""
import itertools

import pytest

from dsd2dxd_amd.shard import shard_range, shard_time

TOTALS = [0, 1, 4095, 24776, 10 ** 7]
WORLDS = [1, 2, 3, 8]
ALIGNS = [1, 4096, 32768]
PREROLLS = [0, 900]


@pytest.mark.parametrize("total,world,align,preroll", list(itertools.product(TOTALS, WORLDS, ALIGNS, PREROLLS)))
def test_slices_tile_the_stream(total, world, align, preroll):
    parts = [shard_time(total, world, r, align=align, preroll=preroll) for r in range(world)]
    at = 0
    for r, (halo, begin, end) in enumerate(parts):
        if end == begin:                                    # an empty slice: the rank sits out
            assert halo == begin
            continue
        assert begin == at, "slices tile [0, total) in rank order"
        assert begin % align == 0 and halo % align == 0
        assert halo <= begin < end
        assert begin - halo >= min(begin, preroll)
        at = end
    assert at == total
    # empty slices only when the stream is too small for the alignment: otherwise every rank has at least `align` bytes of its own
    if total >= world * align:
        assert all(end > begin for _, begin, end in parts)


def test_unaligned_slices_are_shard_ranges():
    for total, world in itertools.product(TOTALS, WORLDS):
        for r in range(world):
            b, e = shard_range(total, world, r)
            halo, begin, end = shard_time(total, world, r)
            if e > b:
                assert (halo, begin, end) == (b, b, e)
            halo, begin, end = shard_time(total, world, r, preroll=900)
            if e > b:
                assert (halo, begin, end) == (max(0, b - 900), b, e)


def test_aligned_example():
    # a DSF file of 10 blocks of 4096 bytes per channel and a ragged tail, over 3 ranks
    total = 10 * 4096 + 123
    assert [shard_time(total, 3, r, align=4096, preroll=900) for r in range(3)] == [
        (0, 0, 3 * 4096), (2 * 4096, 3 * 4096, 6 * 4096), (5 * 4096, 6 * 4096, total)]


def test_last_rank_takes_a_stream_shorter_than_the_alignment():
    assert shard_time(4095, 2, 0, align=4096) == (0, 0, 0)
    assert shard_time(4095, 2, 1, align=4096) == (0, 0, 4095)
    assert shard_time(0, 3, 1) == (0, 0, 0)


@pytest.mark.parametrize("world,rank", [(0, 0), (2, 2), (2, -1), (-1, 0)])
def test_bad_world_or_rank_raises(world, rank):
    with pytest.raises(ValueError):
        shard_time(100, world, rank)
