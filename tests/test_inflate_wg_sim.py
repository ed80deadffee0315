"""The workgroup-per-stream inflate kernel (power-gzip_amd/csrc/nxz_inflate_wg.hip, the product source itself) run on the CPU:
tests/native/hip_cpu_shim.h gives a workgroup an OS thread per lane, barriers, ballots and shuffles, tests/native/inflate_wg_sim.cpp
feeds it streams made by system zlib -- text, zeros, periods, stored blocks, huffman-only, mixed; streams it must hand back (too
long, target too small, cut short, damaged) -- and compares every byte and every result record.  No GPU: this is the check that
the algorithm (pieces in rounds, records, bitmap, resolve) is right before the kernel ever reaches the device."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


PARAMS = [(1, 128, 16)] + ([(2, 160, 1024), (3, 250, 0)] if os.environ.get("NXZ_SIM_FULL") else [])   # (two minutes a run; nres: pieces left in a round up to which a wavefront walks each)


@pytest.mark.skipif(not os.path.exists(CLANG), reason="the kernel source uses clang builtins: needs ROCm's clang++")
@pytest.mark.parametrize("seed,pmin,nres", PARAMS)
def test_workgroup_inflate_kernel_on_the_cpu(tmp_path, seed, pmin, nres):
    exe = tmp_path / "inflate_wg_sim"
    subprocess.run([CLANG, "-O1", "-g", "-std=c++17", "-pthread", os.path.join(ROOT, "tests", "native", "inflate_wg_sim.cpp"),
                    "-o", str(exe), "-lz"], check=True)
    r = subprocess.run([str(exe), os.path.join(ROOT, "tests", "golden", "alice29.txt"), str(seed), str(pmin), str(nres), "70000"],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr


@pytest.mark.skipif(not os.path.exists(CLANG), reason="the kernel source uses clang builtins: needs ROCm's clang++")
# (25 s a run where the default run of the test above takes 15 s: with the other long ones)
@pytest.mark.skipif(not os.environ.get("NXZ_SIM_FULL"), reason="longer than the default run above: set NXZ_SIM_FULL")
@pytest.mark.parametrize("pmin,nres", [(128, 16), (250, 1024)])
def test_hand_built_streams_on_the_cpu(tmp_path, pmin, nres):
    """the streams of tests/deflate_handmade.py as one launch of one workgroup, before they reach the kernel on a device: what
    the kernel takes comes out with the oracle's bytes and record; a stream it hands back is the next kernel's (that counts
    as handed back, not as wrong), and everything that is no whole stream -- an error, a cut, a target too small, a history
    -- must be handed back.  Nothing is written behind a target."""
    import struct

    import deflate_handmade as H
    recs = H.records()
    blob = struct.pack("<I", len(recs))
    for i, c in enumerate(recs):
        blob += struct.pack("<4I", len(c.hist) + len(c.src), len(c.hist), c.cap, (5 * i) % 16) + c.hist + c.src
    (tmp_path / "cases").write_bytes(blob)
    exe = tmp_path / "inflate_wg_sim"
    subprocess.run([CLANG, "-O1", "-g", "-std=c++17", "-pthread", os.path.join(ROOT, "tests", "native", "inflate_wg_sim.cpp"),
                    "-o", str(exe), "-lz"], check=True)
    r = subprocess.run([str(exe), "--cases", str(tmp_path / "cases"), str(tmp_path / "results"), str(pmin), str(nres)],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and r.stdout.strip().endswith("ran"), r.stdout + r.stderr
    got, at, taken = (tmp_path / "results").read_bytes(), 0, []
    for c in recs:
        handed, cc, tpbc, sfbt, subc, spbc, intact = struct.unpack_from("<7I", got, at)
        at += 28
        assert intact, c.name
        whole = not c.err and c.final_eob and not c.hist
        if handed:
            continue
        assert whole, (c.name, "taken: not a whole stream without history")
        assert tpbc == c.tpbc and got[at:at + tpbc] == c.out, c.name
        at += tpbc
        assert (cc, sfbt, subc, spbc) == (0 if c.out_subc < 8 else 3, c.out_sfbt | 0x100, c.out_subc, len(c.src)), (c.name, cc, hex(sfbt), subc, spbc)
        taken.append(c.name)
    assert at == len(got)
    # what the kernel refuses of whole streams is a matter of room (sub-tables, rounds, LDS), never of a rule of the format:
    # most of them it decodes itself, the dynamic blocks of every family among them
    wholes = [c.name for c in recs if not c.err and c.final_eob and not c.hist]
    assert 2 * len(taken) > len(wholes), (len(taken), len(wholes), r.stdout)
    print(r.stdout, sorted(set(wholes) - set(taken)))
