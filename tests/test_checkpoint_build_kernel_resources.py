"""Register, scratch and LDS use of the kernel nxz_batch_checkpoint_build adds, checked by cross-compiling for gfx950
(tools/resource_usage.collect(), no GPU needed).  The kernel is nxzcf::index_kernel's form with a ring of the last 32 KiB of output
beside the walk's tables: no scratch, no spilled vector register, and 40 960 bytes of LDS or fewer, so that four workgroups -- one
wavefront each -- share a CU's 160 KiB.  Measured: nxzcb::build_kernel 105 VGPRs, 39 472 bytes of LDS (the walk's 6704 + 32 768).
The kernels that share the walk without the new hook capability keep their own tests (nxzs::size_kernel, nxzg::index_kernel,
nxzcp::index_kernel, nxzcf::index_kernel): they compile nothing of it."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL = "nxzcb::build_kernel"


@pytest.fixture(scope="module")
def usage():
    spec = importlib.util.spec_from_file_location("resource_usage", os.path.join(ROOT, "tools", "resource_usage.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.collect()


def test_the_namespace_holds_the_one_kernel(usage):
    assert sorted(k for k in usage if k.startswith("nxzcb::")) == [KERNEL]
    assert usage[KERNEL]["file"] == "nxz_checkpoint_build.hip"


def test_no_scratch_no_spill_and_four_workgroups_a_cu(usage):
    u = usage[KERNEL]
    assert u.get("ScratchSize", 0) == 0 and u.get("VGPRs Spill", 0) == 0, u
    assert u["LDS Size"] <= 40960, u
    assert u["LDS Size"] == usage["nxzs::size_kernel"]["LDS Size"] + 32768, u        # the shared walk's tables and stage, and the ring


def test_the_walk_of_the_other_kernels_is_as_it_was(usage):
    """the ring is compiled only for a hook that declares `bytes`: the LDS of the kernels that share the walk is the walk's alone"""
    for k in ("nxzs::size_kernel", "nxzg::index_kernel", "nxzcp::index_kernel", "nxzcf::index_kernel"):
        assert usage[k]["LDS Size"] < 8192 and usage[k].get("ScratchSize", 0) == 0, (k, usage[k])
