"""The block search of the one-stream inflate (power-gzip_amd/csrc/nxz_blockfind.hip, the product source itself:
find_blocks_kernel, check_headers_kernel and both header checkers) run on the CPU: tests/native/hip_cpu_shim.h gives a
workgroup an OS thread per lane, tests/native/blockfind_sim.cpp runs a workgroup per segment over the hand-built headers of
tests/blockfind_cases.py, and what it leaves in `first` is compared with tests/blockfind_model.py: the first header of every
segment exactly, the three further ones exactly where the second kernel does the segment.  No GPU.

Three forms: the two kernels (the default), the first kernel alone (NXZ_BLOCKFIND_TWO=0), and the first kernel with a
wavefront per candidate (header_ok_wave, which the launcher reaches through NXZ_BLOCKFIND_DIAG=5 only; a lane exchange
costs two barriers of 64 threads here, so it gets the cases that are about headers and a few placements)."""
import os
import struct
import subprocess

import pytest

import blockfind_cases as Cs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
TWO, ONE, WAVE = 0, 1, 2


def pack(runs):
    blob = struct.pack("<I", len(runs))
    for c, S, mode in runs:
        blob += struct.pack("<4IQ", len(c.src), c.offset, S, mode, c.first_bit) + c.src
    return blob


def build(tmp_path, source=None):
    exe = tmp_path / "blockfind_sim"
    subprocess.run([CLANG, "-O1", "-g", "-std=c++17", "-pthread", "-I", os.path.join(ROOT, "tests", "native", "hip_sim"),
                    source or os.path.join(ROOT, "tests", "native", "blockfind_sim.cpp"), "-o", str(exe)], check=True)
    return exe


def run(exe, tmp_path, runs):
    """-> what is wrong, a line each"""
    (tmp_path / "cases").write_bytes(pack(runs))
    r = subprocess.run([str(exe), str(tmp_path / "cases")], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and r.stdout.strip().endswith("ran"), r.stdout[-2000:] + r.stderr[-2000:]
    lines = [x.split() for x in r.stdout.splitlines() if x.startswith("case ")]
    assert len(lines) == len(runs)
    bad = []
    for (c, S, mode), x in zip(runs, lines):
        if x[3] != "1":
            bad.append("%s: written outside `first` or the scratch area" % c.name)
        bad += ["%s [%s]" % (b, ("two kernels", "one kernel", "a wavefront per candidate")[mode]) for b in Cs.check(c, S, x[4:], two=mode == TWO)]
    return bad


def wave_cases(S):
    return [c for c in Cs.built(S) if c.name.startswith(("headers-", "the-longest", "ending-at", "cut-", "16-bits", "in-a-last"))]


def runs_for(S):
    return [(c, S, TWO) for c in Cs.built(S)] + [(c, S, ONE) for c in Cs.built(S)] + [(c, S, WAVE) for c in wave_cases(S)]


# (the default run is a subset: segments of 1 KiB -- every case -- and of 2 KiB, where the overflow and the passes of 8192
# positions are; 512 and 8192 bytes run with NXZ_SIM_FULL)
SEGS = Cs.SEGS if os.environ.get("NXZ_SIM_FULL") else (1024, 2048)


@pytest.mark.skipif(not os.path.exists(CLANG), reason="the kernel source uses clang builtins: needs ROCm's clang++")
@pytest.mark.parametrize("S", SEGS)
def test_block_search_on_the_cpu(tmp_path, S):
    bad = run(build(tmp_path), tmp_path, runs_for(S))
    assert not bad, "\n".join(bad[:40])


@pytest.mark.skipif(not os.path.exists(CLANG), reason="the kernel source uses clang builtins: needs ROCm's clang++")
def test_the_header_checkers_alone_on_the_cpu(tmp_path):
    """header_ok (a lane) and header_ok_wave (a wavefront) on every hand-built header at two bit offsets, with nothing in front
    of them to sort out the code-length codes that are not complete.  header_ok leaves that test to the search's first phase
    (its comment says so): it is held to the model for every header but those two; header_ok_wave makes the test itself"""
    import blockfind_model as M
    runs, want = [], []
    for name in Cs.MUST_PASS + Cs.MUST_NOT:
        n = Cs.HEADERS[name][1]
        for bit in (0, 13):
            buf = Cs.filler((bit + n + 7) // 8 + 3, 5)
            Cs.place(buf, bit, name)
            c = Cs.Case(name, bytes(buf), bit, 0, 8192, ())
            runs.append((c, 8192, 3))
            want.append(M.header(M.bits_of(c.src), bit, 8 * len(c.src)))
    (tmp_path / "cases").write_bytes(pack(runs))
    r = subprocess.run([str(build(tmp_path)), str(tmp_path / "cases")], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and r.stdout.strip().endswith("ran"), r.stdout[-2000:] + r.stderr[-2000:]
    lines = [x.split() for x in r.stdout.splitlines() if x.startswith("case ")]
    assert len(lines) == len(runs)
    bad = []
    for (c, _, _), v, x in zip(runs, want, lines):
        if int(x[5]) != v.ok:
            bad.append("%s at bit %d: header_ok_wave %s, the model %s" % (c.name, c.first_bit, x[5], v))
        if v.stage == 2 and int(x[4]) != v.ok:
            bad.append("%s at bit %d: header_ok %s, the model %s" % (c.name, c.first_bit, x[4], v))
    assert not bad, "\n".join(bad)
