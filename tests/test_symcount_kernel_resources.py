"""Register, scratch and LDS use of the symbol-count kernel (nxz_symcount.hip), checked by cross-compiling for gfx950
(tools/resource_usage.collect(), no GPU needed).  It runs between the LZ77 kernel and the table generator with the entropy
kernel's geometry, 256 threads a job: at most 64 VGPRs and no scratch, and 21 KiB of LDS or fewer, so that at least seven
workgroups share a CU and hide one another's loads and LDS atomics.  Measured: 40 VGPRs, 5136 bytes of LDS (a histogram of
320 words a wavefront), eight wavefronts a SIMD.  The LZ77 kernel's forms that count themselves stay in the build
(NXZ_LZ77_COUNT_INKERNEL=1 launches them)."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# kernel -> (max VGPRs, max scratch bytes per lane)
BUDGET = {
    "nxzsc::count_kernel": (64, 0),
}


@pytest.fixture(scope="module")
def usage():
    spec = importlib.util.spec_from_file_location("resource_usage", os.path.join(ROOT, "tools", "resource_usage.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.collect()


def test_the_namespace_holds_the_one_kernel(usage):
    assert sorted(k for k in usage if k.startswith("nxzsc::")) == list(BUDGET)
    assert usage["nxzsc::count_kernel"]["file"] == "nxz_symcount.hip"


def test_registers_scratch_and_seven_workgroups_a_cu(usage):
    for k, (vmax, smax) in BUDGET.items():
        u = usage[k]
        assert u["VGPRs"] <= vmax and u.get("ScratchSize", 0) <= smax and u.get("VGPRs Spill", 0) == 0, (k, u)
        assert u["LDS Size"] <= 21 * 1024, (k, u)


def test_the_lz77_forms_with_and_without_counts_are_both_built(usage):
    for k in ("nxzl77::lz77_kernel<true, false, false>", "nxzl77::lz77_kernel<false, false, false>",
              "nxzl77::lz77_dict_kernel<true, false, false>", "nxzl77::lz77_dict_kernel<false, false, false>"):
        assert k in usage, k
