"""Register and scratch budgets of the kernels nxz_batch_inflate_streams_part adds (power-gzip_amd/csrc/nxz_inflate_part.hip), checked by
cross-compiling for gfx950 (tools/resource_usage.collect(), no GPU needed), and that the kernels of nxz_streams_part.hip -- whose
shift-load function these now share through nxz_shift_load.h -- keep the budgets tests/test_streams_part_kernel_resources.py names.
The budgets are what the compiler reports, rounded up to a multiple of 8; none of the kernels may use scratch or spill, and every one
leaves a SIMD its eight wavefronts:
  open    40 (39 reported): a thread per stream, the header's state machine with one exit (its branches' masks are scalar registers:
          92 of them), the derived job, the table slot copied in a loop that stays a loop;
  stage   32 (32 reported): a binary search, two 16-byte loads and a 128-bit shift, or sixteen byte loads for a piece on a seam;
  close   32 (29 reported): a thread per stream, result and table slot into the carry, the tail byte by byte."""
import importlib.util
import os

import pytest

from test_streams_part_kernel_resources import BUDGET as WRITER

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUDGET = {"nxzip::open_kernel": 40, "nxzip::stage_kernel": 32, "nxzip::close_kernel": 32}


@pytest.fixture(scope="module")
def usage():
    spec = importlib.util.spec_from_file_location("resource_usage", os.path.join(ROOT, "tools", "resource_usage.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.collect()


@pytest.mark.parametrize("kernel", sorted(BUDGET))
def test_inflate_part_kernel_within_budget(usage, kernel):
    assert kernel in usage, sorted(k for k in usage if k.startswith("nxzip::"))
    u = usage[kernel]
    assert u["file"] == "nxz_inflate_part.hip"
    assert u["VGPRs"] <= BUDGET[kernel] and u.get("ScratchSize", 0) == 0 and u.get("VGPRs Spill", 0) == 0, (kernel, u)
    assert u.get("SGPRs Spill", 0) == 0 and u["Occupancy"] == 8, (kernel, u)


def test_the_new_file_holds_exactly_these_kernels(usage):
    assert sorted(k for k, u in usage.items() if u["file"] == "nxz_inflate_part.hip") == sorted(BUDGET)


def test_the_writers_kernels_keep_their_budgets(usage):
    for k, vmax in WRITER.items():
        u = usage[k]
        assert u["file"] == "nxz_streams_part.hip" and u["VGPRs"] <= vmax and u.get("ScratchSize", 0) == 0 and u.get("VGPRs Spill", 0) == 0, (k, u)
        assert u["Occupancy"] == 8, (k, u)
