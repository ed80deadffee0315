"""The BGZF member discovery (power-gzip_amd/csrc/nxz_frame.hip, the product source itself: the two scan passes, tile_scan_kernel,
succ_kernel, jump_kernel, chain_kernel, member_kernel, layout_kernel, coff_kernel) run on the CPU: tests/native/hip_cpu_shim.h
gives a workgroup an OS thread per lane, tests/native/bgzf_discover_sim.cpp runs the launcher's sequence over the hand-built
images of tests/bgzf_discover_cases.py, and everything the launcher promises -- ctl, the candidate list, offsets, the members'
jobs, coff, and what must stay unwritten -- is compared with tests/bgzf_model.py discover().  No GPU.

The model itself is held first: member_size to nxz_bgzf_member_size (tests/native/frame_host.cpp, the code the device runs,
under AddressSanitizer) at every place of every case where the magic stands, and index() to nxz_blocked_scan of libnxz_amd.so,
the product's independent host walk, on every case whose members are real.

The default run leaves out the cases marked `full` (the chains of 1023 members and more, the images of more than 64 KiB):
NXZ_SIM_FULL runs them.  The images of more than 1024 tiles run on the device only (tests/test_gpu_bgzf_discover.py)."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import bgzf_discover_cases as Cs
import bgzf_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
AMD = os.path.join(ROOT, "power-gzip_amd", "libnxz_amd.so")
FULL = bool(os.environ.get("NXZ_SIM_FULL"))
needs_clang = pytest.mark.skipif(not os.path.exists(CLANG), reason="the kernel source uses clang builtins: needs ROCm's clang++")


def sim_cases():
    return [c for c in Cs.cases() if not c.device_only and (FULL or not c.full)]


# ---- the model against the product's host code ----------------------------------------------------------------------------
def test_every_family_has_its_cases():
    fam = Cs.by_family()
    assert all(fam[f] for f in Cs.FAMILIES)
    assert {len(fam["tiles"]), sum(c.device_only for c in Cs.cases())} == {2}
    names = {c.name for c in Cs.cases()}
    for L in Cs.CHAIN_L:
        assert {"chain-%d-members-cap-%d" % (L, L), "chain-%d-members-cap-%d" % (L, L + 1)} <= names
    # the cases say what they are about: the model agrees
    for c in Cs.cases():
        if c.name.startswith("chain-") and c.name.endswith("-cap-%d" % c.cap) and "members" in c.name:
            assert c.model().L == c.max_members and c.model().ctl[0] == c.max_members


def test_member_size_model_against_the_device_code(tmp_path):
    exe = tmp_path / "frame_host"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize=alignment",
                    "-I", os.path.join(ROOT, "power-gzip_amd", "csrc"), os.path.join(ROOT, "tests", "native", "frame_host.cpp"), "-o", str(exe)], check=True)
    recs, want, seen = [], [], set()
    for c in Cs.cases():
        spots, p = [0], c.image.find(M.MAGIC[:3])
        while p >= 0:
            spots.append(p)
            p = c.image.find(M.MAGIC[:3], p + 1)
        spots = sorted(set(spots))
        if len(spots) > 96:                                      # (the images with thousands of headers: the first and the last of them)
            spots = spots[:48] + spots[-48:]
        for p in spots:
            b = c.image[p:p + 66000 if len(c.image) - p > 140000 else len(c.image)]      # (the whole rest, but of the images of megabytes)
            if b in seen:
                continue
            seen.add(b)
            recs.append(bytes([1, 0]) + struct.pack("<I", len(b)) + b)
            want.append((c.name, p, M.member_size(b, 0)))
    r = subprocess.run([str(exe)], input=b"".join(recs), capture_output=True, timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-4000:]
    got = [int(x) for x in r.stdout.decode().splitlines()[1:]]
    assert len(got) == len(want) > 500
    bad = [(n, p, g, w) for (n, p, w), g in zip(want, got) if g != w]
    assert not bad, bad[:20]
    assert sum(1 for _, _, w in want if w) > 100 and sum(1 for _, _, w in want if not w) >= 40


@pytest.mark.skipif(not os.path.exists(AMD), reason="libnxz_amd.so is not built")
def test_index_model_against_the_host_walk():
    L = C.CDLL(AMD)
    L.nxz_blocked_scan.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_size_t)]
    n = 0
    for c in Cs.cases():
        if not c.decodable:
            continue
        m, u, used = C.c_uint64(), C.c_uint64(), C.c_size_t()
        assert L.nxz_blocked_scan(c.image, len(c.image), C.byref(m), C.byref(u), C.byref(used)) == 0
        coff, uoff = M.index(c.image)
        assert (m.value, u.value, used.value) == (len(coff) - 1, uoff[-1], coff[-1]), c.name
        d = M.discover(c.image, 1 << 20, 1 << 20)
        assert (d.L, d.ctl[3], d.used, d.coff, d.offsets) == (len(coff) - 1, uoff[-1], coff[-1], coff, uoff), c.name
        assert sum(len(p) for p in Cs.plains(c)) == uoff[-1]
        n += 1
    assert n == sum(c.decodable for c in Cs.cases()) > 100


# ---- the kernels on the CPU ------------------------------------------------------------------------------------------------
def build(tmp_path, source=None, sanitize=False):
    exe = tmp_path / ("bgzf_discover_sim" + ("_asan" if sanitize else ""))
    subprocess.run([CLANG, "-O1", "-g", "-std=c++17", "-pthread"] + (["-fsanitize=address,undefined", "-fno-sanitize=alignment"] if sanitize else []) +
                   ["-I", os.path.join(ROOT, "tests", "native", "hip_sim"),
                    source or os.path.join(ROOT, "tests", "native", "bgzf_discover_sim.cpp"), "-o", str(exe)], check=True)
    return exe


def simulate(exe, tmp_path, blob, n):
    (tmp_path / "cases").write_bytes(struct.pack("<I", n) + blob)
    r = subprocess.run([str(exe), str(tmp_path / "cases"), str(tmp_path / "out")], capture_output=True, text=True, timeout=1800)
    assert r.returncode == 0 and r.stdout.strip() == "ran %d" % n, r.stdout[-2000:] + r.stderr[-4000:]
    return (tmp_path / "out").read_bytes()


def run(exe, tmp_path, cases):
    """-> what is wrong, a line each"""
    blob = b"".join(struct.pack("<IIIQQ", 0, len(c.image), c.head, c.cap, c.max_members) + c.before + c.image + c.after for c in cases)
    out, at, bad = simulate(exe, tmp_path, blob, len(cases)), 0, []

    def take(dtype, n):
        nonlocal at
        a = np.frombuffer(out, dtype, n, at)
        at += a.nbytes
        return a

    for c in cases:
        ctl, (packed, dst, intact) = take("<u8", 4), take("<u8", 3)
        got = {"ctl": ctl, "packed": int(packed), "dst": int(dst), "guards": {"offsets / coff": bool(intact)}}
        got["pos"], got["size"] = take("<u8", c.cap), take("<u4", c.cap)
        got["offsets"], got["coff"] = take("<u8", c.max_members + 1), take("<u8", c.max_members + 1)
        got["jobs"] = take(Cs.JOB_DTYPE, c.cap)
        bad += Cs.check(c, got)
    assert at == len(out)
    return bad


@needs_clang
def test_discovery_on_the_cpu(tmp_path):
    cases = sim_cases()
    ran = {f: sum(c.family == f for c in cases) for f in Cs.FAMILIES}
    left_out = {f: sum(c.device_only or (c.full and not FULL) for c in v) for f, v in Cs.by_family().items()}
    assert all(ran[f] + left_out[f] == len(v) for f, v in Cs.by_family().items()) and ran["tiles"] == 0
    assert all(ran[f] for f in Cs.FAMILIES if f != "tiles")
    if FULL:
        assert sum(left_out.values()) == 2
    bad = run(build(tmp_path), tmp_path, cases)
    assert not bad, "\n".join(bad[:40])


TILE_COUNTS = (1, 1023, 1024, 1025, 2048, 2049, 5000)


def tile_scan_blob():
    rng = np.random.default_rng(5)
    arrays = [rng.integers(0, 4097, n, dtype=np.uint32) for n in TILE_COUNTS]
    arrays.append(np.full(5000, 4096, np.uint32))
    return arrays, b"".join(struct.pack("<II", 1, len(a)) + a.tobytes() for a in arrays)


def check_tile_scan(out, arrays):
    at = 0
    for a in arrays:
        off = np.frombuffer(out, "<u4", len(a), at)
        total, intact = np.frombuffer(out, "<u8", 2, at + 4 * len(a))
        at += 4 * len(a) + 16
        want = np.cumsum(a.astype(np.uint64))
        assert int(total) == int(want[-1]) and intact == 1, (len(a), int(total), int(want[-1]), int(intact))
        assert (off == (want - a).astype(np.uint32)).all(), len(a)
    assert at == len(out)


@needs_clang
def test_tile_scan_alone_on_the_cpu(tmp_path):
    """tile_scan_kernel on count arrays of 1 .. 5000 tiles (two tiles a lane from 1025 on, five at 5000) against numpy.cumsum;
    behind the counts lies a word that is no count, as in the launcher's workspace"""
    arrays, blob = tile_scan_blob()
    check_tile_scan(simulate(build(tmp_path), tmp_path, blob, len(arrays)), arrays)


@needs_clang
def test_simulation_under_the_sanitizers(tmp_path):
    """the same program with -fsanitize=address,undefined: the workspace is exactly nxz_bgzf_workspace(len, cap) bytes from
    malloc, so an array written or read past its end shows.  The last case of every family and the limits that fill an array to its end, and the
    tile scan on 1025 and 5000 tiles; with NXZ_SIM_FULL every case of the simulation"""
    exe = build(tmp_path, sanitize=True)
    fam = Cs.by_family()
    cases = [[c for c in fam[f] if not c.device_only and not c.full][-1] for f in Cs.FAMILIES if f not in ("tiles", "limits")]
    cases += [c for c in fam["limits"] if c.name in ("limits-candidates-equal-cap", "limits-members-equal-max", "limits-members-max-plus-1")]
    if FULL:
        cases = sim_cases()
    assert len(cases) >= 8
    bad = run(exe, tmp_path, cases)
    assert not bad, "\n".join(bad[:40])
    arrays, _ = tile_scan_blob()
    arrays = [arrays[3], arrays[6]]
    check_tile_scan(simulate(exe, tmp_path, b"".join(struct.pack("<II", 1, len(a)) + a.tobytes() for a in arrays), 2), arrays)
