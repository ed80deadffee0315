"""Register and scratch budgets of the kernels nxz_batch_deflate_streams_dict adds (power-gzip_amd/csrc/nxz_streams_dict.hip), checked by
cross-compiling for gfx950 (tools/resource_usage.collect(), no GPU needed), and that the kernels of nxz_streams.hip -- which now share
their steps with these through nxz_streams_dev.h -- keep their own budgets.  The budgets are what the compiler reports, rounded up
to a multiple of 8; none of the kernels may use scratch or spill:
  prologue_dict / epilogue_dict   24 / 24 (19 / 18 reported): a thread per stream, the plain call's kernels with six header bytes for
                                  two and another bound -- far below the 64 VGPRs at which a SIMD still holds its eight wavefronts;
  expand_dict                     32 (25 reported): expand_kernel's binary search and job record (24) and one more pointer pair for
                                  the second copy of the job in launch order; a thread per block of a chunk, a few thousand threads;
  gather_results                  16 (12 reported): a thread per block copies one 32-byte record through an index."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUDGET = {
    "nxzst::prologue_dict_kernel": 24,
    "nxzst::expand_dict_kernel": 32,
    "nxzst::gather_results_kernel": 16,
    "nxzst::epilogue_dict_kernel": 24,
}
PLAIN = {"nxzst::prologue_kernel": 24, "nxzst::expand_kernel": 24, "nxzst::layout_kernel": 72, "nxzst::pack_kernel": 40, "nxzst::epilogue_kernel": 24}


@pytest.fixture(scope="module")
def usage():
    spec = importlib.util.spec_from_file_location("resource_usage", os.path.join(ROOT, "tools", "resource_usage.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.collect()


@pytest.mark.parametrize("kernel", sorted(BUDGET))
def test_streams_dict_kernel_within_budget(usage, kernel):
    assert kernel in usage, sorted(k for k in usage if k.startswith("nxzst::"))
    u = usage[kernel]
    assert u["file"] == "nxz_streams_dict.hip"
    assert u["VGPRs"] <= BUDGET[kernel] and u.get("ScratchSize", 0) == 0 and u.get("VGPRs Spill", 0) == 0, (kernel, u)
    assert u.get("SGPRs Spill", 0) == 0 and u.get("Occupancy", 8) == 8, (kernel, u)


def test_the_new_file_holds_exactly_these_kernels(usage):
    assert sorted(k for k, u in usage.items() if u["file"] == "nxz_streams_dict.hip") == sorted(BUDGET)


def test_the_plain_calls_kernels_keep_their_budgets(usage):
    for k, vmax in PLAIN.items():
        u = usage[k]
        assert u["file"] == "nxz_streams.hip" and u["VGPRs"] <= vmax and u.get("ScratchSize", 0) == 0 and u.get("VGPRs Spill", 0) == 0, (k, u)
