"""Register and scratch budgets of the kernels the output-size query adds (nxz_batch_decompress_size / _size_framed), checked by
cross-compiling for gfx950 (tools/resource_usage.collect(), no GPU needed).  The walk is the stream-per-wavefront inflate form
without its window and stays inside that form's budget (tests/test_kernel_resources.py): 96 VGPRs, no scratch -- five wavefronts a
SIMD, twenty streams a CU.  Its LDS is the tables alone: below 8 KiB a stream, so LDS (160 KiB a CU) does not hold fewer.  The
trailer step is a small kernel: 64 / 0."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUDGET = {
    "nxzs::size_kernel": (96, 0),
    "nxzs::size_trailer_kernel": (64, 0),
}


@pytest.fixture(scope="module")
def usage():
    spec = importlib.util.spec_from_file_location("resource_usage", os.path.join(ROOT, "tools", "resource_usage.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.collect()


@pytest.mark.parametrize("kernel", sorted(BUDGET))
def test_size_kernel_within_budget(usage, kernel):
    assert kernel in usage, sorted(k for k in usage if "size" in k)
    u = usage[kernel]
    vmax, smax = BUDGET[kernel]
    assert u["VGPRs"] <= vmax and u.get("ScratchSize", 0) <= smax, (kernel, u)


def test_the_walk_keeps_its_tables_and_nothing_else_in_lds(usage):
    u = usage["nxzs::size_kernel"]
    assert u["file"] == "nxz_inflate_size.hip"
    assert u["LDS Size"] <= 8192, u                      # twenty streams a CU need 160 KiB / 20


def test_no_other_kernel_was_added_or_lost_by_the_shared_header(usage):
    """the helpers moved to nxz_inflate_decode.h are still what the decoder's kernels are made of"""
    for k in ("nxzi::inflate_kernel<true, false>", "nxzi::inflate_kernel<false, false>", "nxzi::inflate_dict_kernel",
              "nxzi::block_tables_kernel", "nxzi::token_sync_kernel"):
        assert k in usage and usage[k]["file"] == "nxz_inflate.hip", k
    assert sorted(k for k in usage if k.startswith("nxzs::")) == sorted(BUDGET)
