"""Register and scratch budgets of the kernels nxz_batch_deflate_streams adds (power-gzip_amd/csrc/nxz_streams.hip), checked by
cross-compiling for gfx950 (tools/resource_usage.collect(), no GPU needed), and that moving pack_block into nxz_pack_block.h left
the kernels of nxz_misc.hip in place.  The budgets are what the compiler reports, rounded up to a multiple of 8:
  prologue / expand / epilogue   a thread per stream or block, a few loads and stores: 24 / 24 / 24 -- far below the 64 VGPRs at
                                 which a SIMD still holds its eight wavefronts, which is all a launch of a few thousand threads can use;
  layout                         72 (two 32-step GF(2) products in flight): seven wavefronts a SIMD, where the launch has one
                                 wavefront per stream of a chunk and each waits on a handful of loads -- occupancy is not its limit;
  pack                           40, pack_stream_kernel's figure (tests/test_kernel_resources.py): it is pack_block and two loads."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUDGET = {
    "nxzst::prologue_kernel": 24,
    "nxzst::expand_kernel": 24,
    "nxzst::layout_kernel": 72,
    "nxzst::pack_kernel": 40,
    "nxzst::epilogue_kernel": 24,
}
MISC = ["nxz::dht_prepare_kernel", "nxz::wrap_kernel", "nxz::member_offsets_kernel", "nxz::pack_members_kernel", "nxz::zlib_offsets_kernel",
        "nxz::zlib_dict_offsets_kernel", "nxz::pack_zlib_kernel", "nxz::pack_zlib_dict_kernel", "nxz::stream_offsets_kernel",
        "nxz::pack_stream_kernel", "nxz::member_stream_offsets_kernel", "nxz::member_pack_stream_kernel", "nxz::sample_btype_kernel"]


@pytest.fixture(scope="module")
def usage():
    spec = importlib.util.spec_from_file_location("resource_usage", os.path.join(ROOT, "tools", "resource_usage.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.collect()


@pytest.mark.parametrize("kernel", sorted(BUDGET))
def test_streams_kernel_within_budget(usage, kernel):
    assert kernel in usage, sorted(k for k in usage if k.startswith("nxzst::"))
    u = usage[kernel]
    assert u["file"] == "nxz_streams.hip"
    assert u["VGPRs"] <= BUDGET[kernel] and u.get("ScratchSize", 0) == 0 and u.get("VGPRs Spill", 0) == 0, (kernel, u)


def test_the_new_file_holds_exactly_these_kernels(usage):
    assert sorted(k for k, u in usage.items() if u["file"] == "nxz_streams.hip") == sorted(BUDGET)


def test_the_kernels_of_nxz_misc_are_still_there(usage):
    for k in MISC:
        assert k in usage and usage[k]["file"] == "nxz_misc.hip", k
    # the two that are made of pack_block keep their registers (34 before the move) and use no scratch
    for k in ("nxz::pack_stream_kernel", "nxz::member_pack_stream_kernel"):
        assert usage[k]["VGPRs"] <= 40 and usage[k].get("ScratchSize", 0) == 0, usage[k]
