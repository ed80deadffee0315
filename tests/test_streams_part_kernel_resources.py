"""Register and scratch budgets of the kernels nxz_batch_deflate_streams_part adds (power-gzip_amd/csrc/nxz_streams_part.hip), checked by
cross-compiling for gfx950 (tools/resource_usage.collect(), no GPU needed), and that the kernels of nxz_streams.hip -- whose layout
step these now share through nxz_streams_dev.h -- keep the budgets tests/test_streams_dict_kernel_resources.py names.  The budgets are
what the compiler reports, rounded up to a multiple of 8; none of the kernels may use scratch or spill, and every one leaves a SIMD
its eight wavefronts:
  prologue / epilogue   32 / 32 (28 / 32 reported): a thread per stream, the plain call's kernels with a 48-byte descriptor and the
                        32-byte carry record read (and, in the epilogue, written back) beside the state;
  expand                24 (24 reported): expand_kernel's binary search and job record, one more load for the staging slot;
  stage                 16 (14 reported): a workgroup per staged block, two 16-byte loads and a 128-bit shift in flight;
  layout                64 (64 reported): layout_stream, as nxz_streams.hip's layout_kernel;
  pack                  40 (34 reported): pack_block and three loads, as nxz_streams.hip's pack_kernel."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUDGET = {
    "nxzsp::prologue_kernel": 32,
    "nxzsp::expand_kernel": 24,
    "nxzsp::stage_kernel": 16,
    "nxzsp::layout_kernel": 64,
    "nxzsp::pack_kernel": 40,
    "nxzsp::epilogue_kernel": 32,
}
PLAIN = {"nxzst::prologue_kernel": 24, "nxzst::expand_kernel": 24, "nxzst::layout_kernel": 72, "nxzst::pack_kernel": 40, "nxzst::epilogue_kernel": 24}


@pytest.fixture(scope="module")
def usage():
    spec = importlib.util.spec_from_file_location("resource_usage", os.path.join(ROOT, "tools", "resource_usage.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.collect()


@pytest.mark.parametrize("kernel", sorted(BUDGET))
def test_streams_part_kernel_within_budget(usage, kernel):
    assert kernel in usage, sorted(k for k in usage if k.startswith("nxzsp::"))
    u = usage[kernel]
    assert u["file"] == "nxz_streams_part.hip"
    assert u["VGPRs"] <= BUDGET[kernel] and u.get("ScratchSize", 0) == 0 and u.get("VGPRs Spill", 0) == 0, (kernel, u)
    assert u.get("SGPRs Spill", 0) == 0 and u["Occupancy"] == 8, (kernel, u)


def test_the_new_file_holds_exactly_these_kernels(usage):
    assert sorted(k for k, u in usage.items() if u["file"] == "nxz_streams_part.hip") == sorted(BUDGET)


def test_the_plain_calls_kernels_keep_their_budgets(usage):
    for k, vmax in PLAIN.items():
        u = usage[k]
        assert u["file"] == "nxz_streams.hip" and u["VGPRs"] <= vmax and u.get("ScratchSize", 0) == 0 and u.get("VGPRs Spill", 0) == 0, (k, u)
    assert sorted(k for k, u in usage.items() if u["file"] == "nxz_streams.hip") == sorted(PLAIN)
