"""d2d_segments_move_device and d2d_segments_pack_device (include/dsd2dxd_amd.h, "A chunk's bookkeeping in one launch") on the GPU:
the cases of tests/segments_cases.py, which tests/test_segments_cpu.py runs through the host twins, with device and pinned memory on
either side.  Whole arenas are compared with a numpy model: every byte of a range equals its source, every byte outside -- 256 guard
bytes around each range included -- is what it was, under two complementary fills.  One call of the move cases holds 2840 segments, 30
launches of 96."""
import numpy as np
import pytest

import segments_cases as S

gpu = pytest.mark.gpu


class TorchMemory:
    """device tensors, or pinned host tensors the GPU addresses in place"""

    def __init__(self, pinned):
        self.pinned = pinned

    def alloc(self, nbytes):
        import torch
        t = torch.zeros(nbytes + 16, dtype=torch.uint8)
        t = t.pin_memory() if self.pinned else t.cuda()
        off = (-t.data_ptr()) % 16
        v = t[off:off + nbytes]

        def read():
            torch.cuda.synchronize()
            return v.cpu().numpy().copy()

        def write(x):
            v.copy_(torch.from_numpy(np.ascontiguousarray(x)))
            torch.cuda.synchronize()

        return S.Buffer(v.data_ptr(), read, write, keep=t)

    def sync(self):
        import torch
        torch.cuda.synchronize()


KINDS = {"device": False, "pinned": True}


@gpu
@pytest.mark.parametrize("fill", S.FILLS)
@pytest.mark.parametrize("dst_kind", KINDS)
@pytest.mark.parametrize("src_kind", KINDS)
def test_move_writes_the_ranges_and_nothing_else(engine_lib, src_kind, dst_kind, fill):
    S.check_move(engine_lib, engine_lib.segments_move_device, TorchMemory(KINDS[src_kind]), TorchMemory(KINDS[dst_kind]), fill)


@gpu
def test_move_refuses_overlap_and_changes_nothing(engine_lib):
    S.check_move_refusals(engine_lib, engine_lib.segments_move_device, TorchMemory(False))


@gpu
@pytest.mark.parametrize("fill", S.FILLS)
@pytest.mark.parametrize("dst_kind", KINDS)
@pytest.mark.parametrize("case", ["few", "many"])
def test_pack_lays_the_segments_back_to_back(engine_lib, case, dst_kind, fill):
    """the lengths lie in device memory and are read there; the destination and the table are device or pinned memory"""
    S.check_pack(engine_lib, engine_lib.segments_pack_device, TorchMemory(False), TorchMemory(KINDS[dst_kind]), case, fill)


@gpu
@pytest.mark.parametrize("case,too_long", [("few", 2), ("few", 0), ("many", 5), ("many", 299)])
def test_pack_with_a_length_above_its_maximum_writes_only_the_table(engine_lib, case, too_long):
    """... in the first launch of a cut call and in its last: every entry of the table is UINT64_MAX, no byte of dst changes"""
    S.check_pack(engine_lib, engine_lib.segments_pack_device, TorchMemory(False), TorchMemory(True), case, S.FILLS[1], too_long=too_long)


@gpu
def test_pack_of_nothing_and_refusals(engine_lib):
    S.check_pack_empty_and_refusals(engine_lib, engine_lib.segments_pack_device, TorchMemory(False))
    d, mem = engine_lib, TorchMemory(False)
    table, lens = mem.alloc(24), mem.alloc(8)
    srcs = (d.PackSrc * 1)()
    srcs[0].base, srcs[0].bytes, srcs[0].max_bytes = lens.ptr, lens.ptr, 8
    with pytest.raises(d.D2DError) as ex:                                  # the device call wants the table 8-byte aligned
        d.segments_pack_device(srcs, table.ptr, 8, table.ptr + 4)
    assert ex.value.code == S.ERR_PARAM
