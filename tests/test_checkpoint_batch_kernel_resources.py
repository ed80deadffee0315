"""Register, scratch and LDS use of the kernels the batched range read adds (nxz_batch_checkpoint_read_ranges), checked by
cross-compiling for gfx950 (tools/resource_usage.collect(), no GPU needed).  None of them uses scratch or spills a vector register,
and the only LDS is what the bases' prefix sum needs: the sums of the sixteen wavefronts of its one workgroup, 16 x 8 = 128 bytes
(inside a wavefront the sum goes through shuffles).
Measured: nxzcr::rows_kernel 24 VGPRs, nxzcr::base_kernel 52 VGPRs and 128 bytes of LDS, nxzcr::flat_kernel 13, nxzcr::status_kernel
12, nxzcr::stage_kernel 12; no LDS in any but base_kernel."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ["nxzcr::rows_kernel", "nxzcr::base_kernel", "nxzcr::flat_kernel", "nxzcr::status_kernel", "nxzcr::stage_kernel"]
SCAN_LDS = 16 * 8


@pytest.fixture(scope="module")
def usage():
    spec = importlib.util.spec_from_file_location("resource_usage", os.path.join(ROOT, "tools", "resource_usage.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.collect()


@pytest.mark.parametrize("kernel", KERNELS)
def test_batch_kernel_uses_no_scratch_and_no_lds_beyond_the_scan(usage, kernel):
    assert kernel in usage, sorted(k for k in usage if k.startswith("nxzcr::"))
    u = usage[kernel]
    assert u["file"] == "nxz_checkpoint_batch.hip"
    assert u.get("ScratchSize", 0) == 0 and u.get("VGPRs Spill", 0) == 0, (kernel, u)
    assert u["VGPRs"] <= 64, (kernel, u)
    assert u["LDS Size"] == (SCAN_LDS if kernel == "nxzcr::base_kernel" else 0), (kernel, u)


def test_no_other_kernel_in_the_namespace(usage):
    assert sorted(k for k in usage if k.startswith("nxzcr::")) == sorted(KERNELS)
