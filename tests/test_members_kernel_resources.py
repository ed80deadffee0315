"""Register, scratch and LDS budgets of the kernels the multi-member gzip calls add (nxz_batch_gzip_members_size / _decode), checked
by cross-compiling for gfx950 (tools/resource_usage.collect(), no GPU needed).  The index kernel is the size walk's form
(tests/test_size_kernel_resources.py) in a loop over the members of a job, with the header parser in front of every walk: the same
budget -- 96 VGPRs, no scratch, five wavefronts a SIMD -- and the walk's LDS (at most 8 KiB) plus what the parser needs.
Measured: 85 VGPRs, 0 bytes of scratch, 6704 bytes of LDS -- the walk's 6704 to the byte: the parsed header lives in registers,
the parser takes no LDS at all, so its allowance is 0.  The decode's plumbing is small kernels: 64 / 0."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARSER_LDS = 0
BUDGET = {
    "nxzg::index_kernel": (96, 0),
    "nxzg::check_kernel": (64, 0),
    "nxzg::plan_kernel": (64, 0),
    "nxzg::fill_kernel": (64, 0),
    "nxzg::expand_kernel": (64, 0),
    "nxzg::join_kernel": (64, 0),
    "nxzg::finish_kernel": (64, 0),
}


@pytest.fixture(scope="module")
def usage():
    spec = importlib.util.spec_from_file_location("resource_usage", os.path.join(ROOT, "tools", "resource_usage.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.collect()


@pytest.mark.parametrize("kernel", sorted(BUDGET))
def test_members_kernel_within_budget(usage, kernel):
    assert kernel in usage, sorted(k for k in usage if k.startswith("nxzg::"))
    u = usage[kernel]
    vmax, smax = BUDGET[kernel]
    assert u["file"] == "nxz_gzip_members.hip"
    assert u["VGPRs"] <= vmax and u.get("ScratchSize", 0) <= smax, (kernel, u)


def test_the_index_keeps_the_walks_lds(usage):
    u, walk = usage["nxzg::index_kernel"], usage["nxzs::size_kernel"]
    assert u["LDS Size"] <= 8192 + PARSER_LDS, u
    assert u["LDS Size"] <= walk["LDS Size"] + PARSER_LDS, (u, walk)     # the shared walk's tables and stage, nothing of its own


def test_no_other_kernel_in_the_namespace(usage):
    assert sorted(k for k in usage if k.startswith("nxzg::")) == sorted(BUDGET)
