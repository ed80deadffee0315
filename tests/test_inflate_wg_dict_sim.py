"""The dictionary form of the workgroup-per-stream inflate kernel (nxzw::inflate_wg_dict_kernel, power-gzip_amd/csrc/nxz_inflate_wg.hip,
the product source itself) run on the CPU through tests/native/hip_cpu_shim.h: tests/native/inflate_wg_dict_sim.cpp feeds it raw
deflate streams that system zlib made with deflateSetDictionary -- levels 1, 6 and 9, records of 1 byte to 300 KiB, dictionaries of
1, 17, 4 099, 32 768 and 50 000 bytes and none, a record equal to the dictionary, a record without references, a job that says
NXZ_JOB_NO_DICT -- and compares every output byte and result; the streams the kernel must not decode (a distance in front of the
window, cut short, target too small) must be on the hand-back list.  No GPU: this is the check that the preloaded window and
the state around it are right before the kernel reaches the device."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"

PARAMS = [(1, 128)] + ([(2, 160), (3, 250)] if os.environ.get("NXZ_SIM_FULL") else [])


@pytest.mark.skipif(not os.path.exists(CLANG), reason="the kernel source uses clang builtins: needs ROCm's clang++")
@pytest.mark.parametrize("seed,pmin", PARAMS)
def test_workgroup_inflate_kernel_with_a_dictionary_on_the_cpu(tmp_path, seed, pmin):
    exe = tmp_path / "inflate_wg_dict_sim"
    subprocess.run([CLANG, "-O1", "-g", "-std=c++17", "-pthread", os.path.join(ROOT, "tests", "native", "inflate_wg_dict_sim.cpp"),
                    "-o", str(exe), "-lz"], check=True)
    r = subprocess.run([str(exe), os.path.join(ROOT, "tests", "golden", "alice29.txt"), str(seed), str(pmin), str(300 * 1024)],
                       capture_output=True, text=True, timeout=1800)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr
