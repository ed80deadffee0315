"""Register, scratch and LDS use of the kernels the fine checkpoint calls add (nxz_batch_checkpoint_index_fine /
nxz_checkpoint_read_ranges_fine), checked by cross-compiling for gfx950 (tools/resource_usage.collect(), no GPU needed).  None of
them uses scratch or spills a vector register (the index kernel keeps some scalars in vector lanes, as the size kernel and both
other index kernels do).  The index kernel is nxzcp::index_kernel's form with a hook that cuts between tokens: its LDS is the shared
walk's, and at 96 VGPRs or fewer it keeps the five wavefronts a SIMD that the member index kernel has at 85.
Measured: nxzcf::index_kernel 72 VGPRs, 6704 bytes of LDS (nxzs::size_kernel 72 / 6704, nxzcp::index_kernel 69 / 6704);
nxzcf::check_kernel 14 VGPRs, nxzcf::jobs_kernel 12 VGPRs, no LDS."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ["nxzcf::index_kernel", "nxzcf::check_kernel", "nxzcf::jobs_kernel"]


@pytest.fixture(scope="module")
def usage():
    spec = importlib.util.spec_from_file_location("resource_usage", os.path.join(ROOT, "tools", "resource_usage.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.collect()


@pytest.mark.parametrize("kernel", KERNELS)
def test_fine_checkpoint_kernel_uses_no_scratch(usage, kernel):
    assert kernel in usage, sorted(k for k in usage if k.startswith("nxzcf::"))
    u = usage[kernel]
    assert u["file"] == "nxz_checkpoint_fine.hip"
    assert u.get("ScratchSize", 0) == 0 and u.get("VGPRs Spill", 0) == 0, (kernel, u)
    if kernel != "nxzcf::index_kernel":
        assert u["VGPRs"] <= 64 and u["LDS Size"] == 0, (kernel, u)


def test_the_fine_index_keeps_five_wavefronts_a_simd(usage):
    u = usage["nxzcf::index_kernel"]
    assert u["VGPRs"] <= 96, u
    assert u["LDS Size"] <= usage["nxzs::size_kernel"]["LDS Size"], u           # the shared walk's tables and stage, nothing of its own


def test_no_other_kernel_in_the_namespace(usage):
    assert sorted(k for k in usage if k.startswith("nxzcf::")) == sorted(KERNELS)
