"""Register and scratch budgets of the kernels the shared preset dictionary adds (nxz_batch_*_dict), checked by cross-compiling for
gfx950 (tools/resource_usage.collect(), no GPU needed).  Each new entry point runs the body of an existing kernel and stays inside
that kernel's budget (tests/test_kernel_resources.py): the LZ77 forms 128 VGPRs / 64 bytes of scratch, the workgroup inflate form
128 / 128, the stream-per-wavefront form 96 / 0 (five wavefronts per SIMD); the small kernels around them 64 / 0."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUDGET = {
    "nxzl77::lz77_dict_kernel<false, false, false>": (128, 64),
    "nxzl77::lz77_dict_kernel<true, false, false>": (128, 64),
    "nxzl77::lz77_dict_kernel<false, true, false>": (128, 64),
    "nxzl77::lz77_dict_kernel<true, false, true>": (128, 64),
    "nxzw::inflate_wg_dict_kernel<false>": (128, 128),
    "nxzi::inflate_dict_kernel": (96, 0),
    "nxzl77::dict_jobs_kernel": (64, 0),
    "nxzl77::dict_finish_kernel": (64, 0),
    "nxz::pack_zlib_dict_kernel": (64, 0),
    "nxz::zlib_dict_offsets_kernel": (64, 0),
    "nxzf::frame_header_dict_kernel": (64, 0),
}


@pytest.fixture(scope="module")
def usage():
    spec = importlib.util.spec_from_file_location("resource_usage", os.path.join(ROOT, "tools", "resource_usage.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.collect()


@pytest.mark.parametrize("kernel", sorted(BUDGET))
def test_dict_kernel_within_budget(usage, kernel):
    assert kernel in usage, sorted(k for k in usage if "dict" in k)
    u = usage[kernel]
    vmax, smax = BUDGET[kernel]
    assert u["VGPRs"] <= vmax and u.get("ScratchSize", 0) <= smax, (kernel, u)
