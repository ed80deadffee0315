"""Register, scratch and LDS use of the kernel the batched verify adds (nxz_batch_decompress_verify / _verify_framed), checked by
cross-compiling for gfx950 (tools/resource_usage.collect(), no GPU needed).  The kernel is nxzcb::build_kernel's form -- the shared
walk with a ring of the last 32 KiB of output -- plus a slice-by-4 CRC table of 4 KiB in LDS: no scratch, no spilled vector
register, and 54 613 bytes of LDS or fewer, so that three workgroups -- one wavefront each -- share a CU's 160 KiB.  Measured:
nxzv::verify_kernel 149 VGPRs, 43 568 bytes of LDS (the walk's 6704 + 32 768 + 4096).  The kernels that share the walk or the
ring's writers keep the LDS their own tests pin."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL = "nxzv::verify_kernel"


@pytest.fixture(scope="module")
def usage():
    spec = importlib.util.spec_from_file_location("resource_usage", os.path.join(ROOT, "tools", "resource_usage.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.collect()


def test_the_namespace_holds_the_one_kernel(usage):
    assert sorted(k for k in usage if k.startswith("nxzv::")) == [KERNEL]
    assert usage[KERNEL]["file"] == "nxz_inflate_verify.hip"


def test_no_scratch_no_spill_and_three_workgroups_a_cu(usage):
    u = usage[KERNEL]
    assert u.get("ScratchSize", 0) == 0 and u.get("VGPRs Spill", 0) == 0, u
    assert u["LDS Size"] <= 54613, u                                                     # 160 KiB / 3
    walk = usage["nxzs::size_kernel"]["LDS Size"]
    assert walk + 32768 <= u["LDS Size"] <= walk + 32768 + 4096, u                       # the walk, the ring, at most a 4 KiB table


def test_the_kernels_that_share_the_walk_and_the_ring_are_as_they_were(usage):
    walk = usage["nxzs::size_kernel"]["LDS Size"]
    assert walk == 6704
    assert usage["nxzcb::build_kernel"]["LDS Size"] == walk + 32768
    assert usage["nxzcb::build_kernel"].get("ScratchSize", 0) == 0 and usage["nxzcb::build_kernel"].get("VGPRs Spill", 0) == 0
    for k in ("nxzs::size_kernel", "nxzg::index_kernel", "nxzcp::index_kernel", "nxzcf::index_kernel"):
        assert usage[k]["LDS Size"] < 8192 and usage[k].get("ScratchSize", 0) == 0, (k, usage[k])
