"""Register and scratch budgets of the BGZF range kernels (power-gzip_amd/csrc/nxz_bgzf.hip) and of the index kernel nxz_bgzf_index
adds to nxz_frame.hip, checked by cross-compiling for gfx950 (tools/resource_usage.collect(), no GPU needed).  They are small
kernels: at most 64 VGPRs (eight waves per SIMD) and no scratch."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ["nxzr::index_check_kernel", "nxzr::range_map_kernel", "nxzr::member_scan_kernel", "nxzr::range_scan_kernel",
           "nxzr::job_kernel", "nxzr::gather_kernel", "nxzr::zero_kernel", "nxzf::coff_kernel"]


@pytest.fixture(scope="module")
def usage():
    spec = importlib.util.spec_from_file_location("resource_usage", os.path.join(ROOT, "tools", "resource_usage.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.collect()


@pytest.mark.parametrize("kernel", KERNELS)
def test_bgzf_kernel_within_budget(usage, kernel):
    assert kernel in usage, sorted(k for k in usage if k.startswith(("nxzr", "nxzf")))
    u = usage[kernel]
    assert u["VGPRs"] <= 64 and u.get("ScratchSize", 0) == 0, (kernel, u)
