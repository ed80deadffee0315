"""Register, scratch and LDS budgets of the kernels nxz_batch_shuffle / nxz_batch_unshuffle add (power-gzip_amd/csrc/nxz_shuffle.hip),
checked by cross-compiling for gfx950 (tools/resource_usage.collect(), no GPU needed).  The budgets are what the compiler reports,
rounded up to a multiple of 8; none of the kernels may use scratch or spill:
  shuffle_kernel<false>   48 (44 reported): the five bodies (elem 2, 4, 8, 16, generic) in one kernel, 16 source bytes a lane scattered;
  shuffle_kernel<true>    32 (32 reported): the same with 16 bytes a lane gathered;
  shuffle_status_kernel    8 ( 4 reported).
LDS: the planes of a tile and the plane table, what nxz_shuffle.h names NXZ_SHUFFLE_LDS_BYTES (21 504 bytes: seven workgroups a
compute unit, which is what bounds the two tile kernels at seven wavefronts a SIMD)."""
import importlib.util
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUDGET = {"nxzsh::shuffle_kernel<false>": 48, "nxzsh::shuffle_kernel<true>": 32, "nxzsh::shuffle_status_kernel": 8}


def header_value(name):
    """a #define of nxz_shuffle.h / nxz_engine.h, evaluated (sums and products of numbers and other defines)"""
    text = open(os.path.join(ROOT, "power-gzip_amd", "csrc", "nxz_shuffle.h")).read() + open(os.path.join(ROOT, "include", "nxz_engine.h")).read()
    m = re.search(r"^#define %s\s+(.+?)\s*(/\*.*)?$" % name, text, re.M)
    assert m, name
    expr = re.sub(r"\b(\d+)u\b", r"\1", m.group(1))
    expr = re.sub(r"\bNXZ_\w+", lambda n: str(header_value(n.group(0))), expr)
    assert re.fullmatch(r"[\d\s()+*]+", expr), expr
    return eval(expr)


@pytest.fixture(scope="module")
def usage():
    spec = importlib.util.spec_from_file_location("resource_usage", os.path.join(ROOT, "tools", "resource_usage.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.collect()


@pytest.mark.parametrize("kernel", sorted(BUDGET))
def test_shuffle_kernel_within_budget(usage, kernel):
    assert kernel in usage, sorted(k for k in usage if k.startswith("nxzsh::"))
    u = usage[kernel]
    assert u["file"] == "nxz_shuffle.hip"
    assert u["VGPRs"] <= BUDGET[kernel] and u.get("ScratchSize", 0) == 0 and u.get("VGPRs Spill", 0) == 0, (kernel, u)
    assert u.get("SGPRs Spill", 0) == 0 and u["Occupancy"] >= 7, (kernel, u)


def test_lds_is_what_the_header_claims(usage):
    claim = header_value("NXZ_SHUFFLE_LDS_BYTES")
    assert claim == 16384 + 16 * 256 + 4 * 256
    for k in BUDGET:
        want = claim if "shuffle_kernel" in k else 0
        assert usage[k].get("LDS Size", 0) <= want, (k, usage[k])
    assert usage["nxzsh::shuffle_kernel<false>"]["LDS Size"] == usage["nxzsh::shuffle_kernel<true>"]["LDS Size"] == claim


def test_the_new_file_holds_exactly_these_kernels(usage):
    assert sorted(k for k, u in usage.items() if u["file"] == "nxz_shuffle.hip") == sorted(BUDGET)
