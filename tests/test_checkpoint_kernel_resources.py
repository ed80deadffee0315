"""Register, scratch and LDS use of the kernels the checkpoint calls add (nxz_batch_checkpoint_index / nxz_checkpoint_read_ranges),
checked by cross-compiling for gfx950 (tools/resource_usage.collect(), no GPU needed).  None of them uses scratch.  The index kernel
is the size walk with the header parser in front and a hook at every block header -- the member index kernel's form without its
loop over members -- and stays inside that kernel's VGPR and LDS figures, whatever they are in this tree.  Measured: 69 VGPRs,
6704 bytes of LDS (the member index kernel: 85 / 6704).  The plumbing is small kernels without LDS."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ["nxzcp::index_kernel", "nxzcp::window_kernel", "nxzcp::check_kernel", "nxzcp::inmax_kernel", "nxzcp::stage_kernel", "nxzcp::verdict_kernel"]


@pytest.fixture(scope="module")
def usage():
    spec = importlib.util.spec_from_file_location("resource_usage", os.path.join(ROOT, "tools", "resource_usage.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.collect()


@pytest.mark.parametrize("kernel", KERNELS)
def test_checkpoint_kernel_uses_no_scratch(usage, kernel):
    assert kernel in usage, sorted(k for k in usage if k.startswith("nxzcp::"))
    u = usage[kernel]
    assert u["file"] == "nxz_checkpoint.hip"
    assert u.get("ScratchSize", 0) == 0 and u.get("VGPRs Spill", 0) == 0, (kernel, u)
    if kernel != "nxzcp::index_kernel":
        assert u["VGPRs"] <= 64 and u["LDS Size"] == 0, (kernel, u)


def test_the_index_stays_inside_the_member_index(usage):
    u, members = usage["nxzcp::index_kernel"], usage["nxzg::index_kernel"]
    assert u["VGPRs"] <= members["VGPRs"] and u["LDS Size"] <= members["LDS Size"], (u, members)
    assert u["LDS Size"] <= usage["nxzs::size_kernel"]["LDS Size"], u           # the shared walk's tables and stage, nothing of its own


def test_no_other_kernel_in_the_namespace(usage):
    assert sorted(k for k in usage if k.startswith("nxzcp::")) == sorted(KERNELS)
