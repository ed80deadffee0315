"""Register and scratch budgets of the kernels nxz_batch_deflate_streams_indexed adds (power-gzip_amd/csrc/nxz_streams_index.hip), checked
by cross-compiling for gfx950 (tools/resource_usage.collect(), no GPU needed).  The budgets are what the compiler reports, rounded up
to a multiple of 8:
  prologue / epilogue   8 / 24 (reported 8 / 20): a thread per stream, a few loads and stores;
  sweep                 32 (reported 28): two headers a lane as four 64-bit values, two ballots and a shuffle a step;
  windows               56 (reported 54): the 16-byte copy unrolled, up to eight uint4 in flight a lane.
All four lie below the 64 VGPRs at which a SIMD still holds its eight wavefronts, so none limits occupancy: the compiler reports
occupancy 8 for each, which the test asks for as well.  No kernel uses scratch, spills or LDS.  The kernels of nxz_streams.hip,
nxz_streams_dict.hip and nxz_misc.hip are pinned by their own tests (tests/test_streams_kernel_resources.py,
tests/test_streams_dict_kernel_resources.py), which pass unchanged: the new file left them alone."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUDGET = {
    "nxzsi::prologue_kernel": 8,
    "nxzsi::sweep_kernel": 32,
    "nxzsi::window_kernel": 56,
    "nxzsi::epilogue_kernel": 24,
}


@pytest.fixture(scope="module")
def usage():
    spec = importlib.util.spec_from_file_location("resource_usage", os.path.join(ROOT, "tools", "resource_usage.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.collect()


@pytest.mark.parametrize("kernel", sorted(BUDGET))
def test_streams_index_kernel_within_budget(usage, kernel):
    assert kernel in usage, sorted(k for k in usage if k.startswith("nxzsi::"))
    u = usage[kernel]
    assert u["file"] == "nxz_streams_index.hip"
    assert u["VGPRs"] <= BUDGET[kernel] and u.get("ScratchSize", 0) == 0 and u.get("VGPRs Spill", 0) == 0 and u.get("SGPRs Spill", 0) == 0, (kernel, u)
    assert u.get("LDS Size", 0) == 0 and u["Occupancy"] == 8, (kernel, u)


def test_the_new_file_holds_exactly_these_kernels(usage):
    assert sorted(k for k, u in usage.items() if u["file"] == "nxz_streams_index.hip") == sorted(BUDGET)
