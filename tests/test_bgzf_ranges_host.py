"""BGZF random access without a GPU: the range mapping the device runs (power-gzip_amd/csrc/nxz_bgzf_range.h) compiled for the
host under AddressSanitizer and compared with a Python model (tests/bgzf_model.py) on random indexes, and the .gzi functions of
libnxz_amd.so (nxz_gzi_write / nxz_gzi_read) against a Python struct writer and reader."""
import ctypes as C
import os
import random
import struct
import subprocess

import pytest

import bgzf_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "power-gzip_amd", "libnxz_amd.so")


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    exe = tmp_path_factory.mktemp("bgzf") / "bgzf_range_host"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize=alignment",
                    "-I", os.path.join(ROOT, "power-gzip_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "bgzf_range_host.cpp"), "-o", str(exe)], check=True)

    def run(cases):
        """cases: [(coff, uoff, [(kind, b, e), ...])] -> per case, a list of (status, ub, ue, first, last)"""
        blob = b""
        for coff, uoff, qs in cases:
            blob += struct.pack("<Q", len(coff) - 1) + struct.pack("<%dQ" % len(coff), *coff) + struct.pack("<%dQ" % len(uoff), *uoff)
            blob += struct.pack("<Q", len(qs)) + b"".join(struct.pack("<QQQ", k, b, e) for k, b, e in qs)
        r = subprocess.run([str(exe)], input=blob, capture_output=True, timeout=600)
        assert r.returncode == 0, r.stderr.decode()[-4000:]
        lines = iter(r.stdout.decode().splitlines())
        return [[tuple(int(x) for x in next(lines).split()) for _ in qs] for _, _, qs in cases]
    return run


def random_index(rnd, members, base_c=0, base_u=0):
    """members with runs of empty ones, an end marker at the end; compressed sizes >= 28"""
    coff, uoff = [base_c], [base_u]
    for j in range(members):
        kind = rnd.random()
        isize = 0 if kind < 0.15 else rnd.choice([1, 2, 65280, 65536, rnd.randrange(1, 70000)])
        if kind < 0.05:                      # a run of empty members
            for _ in range(rnd.randrange(1, 4)):
                coff.append(coff[-1] + 28)
                uoff.append(uoff[-1])
        coff.append(coff[-1] + rnd.randrange(28, 65537))
        uoff.append(uoff[-1] + isize)
    coff.append(coff[-1] + 28)               # the end marker
    uoff.append(uoff[-1])
    return coff, uoff


def queries(rnd, coff, uoff):
    L, U = len(coff) - 1, uoff[-1]
    q = []
    cuts = sorted(set(uoff))
    for _ in range(200):
        b = rnd.randrange(uoff[0], U + 1)
        e = rnd.randrange(b, U + 1)
        q.append((M.UOFF, b, e))
    for c in cuts:                               # member boundaries, empty ranges, ends
        q += [(M.UOFF, c, c), (M.UOFF, c, min(U, c + 1)), (M.UOFF, max(uoff[0], c - 1), c), (M.UOFF, uoff[0], c), (M.UOFF, c, U)]
    q += [(M.UOFF, uoff[0], U), (M.UOFF, U, U), (M.UOFF, U, U + 1), (M.UOFF, U - 1 if U else 0, U), (M.UOFF, 5, 4),
          (M.UOFF, U + 1, U + 2), (M.UOFF, 0, 1 << 63)]
    if uoff[0]:
        q += [(M.UOFF, uoff[0] - 1, uoff[0]), (M.UOFF, 0, 0)]
    # virtual offsets: at member starts, inside, at within == ISIZE, past it, a coff that is no member start, the end
    for j in range(L + 1):
        isize = uoff[j + 1] - uoff[j] if j < L else 0
        for w in {0, isize // 2, isize, isize + 1, min(0xffff, isize + 1)}:
            if w <= 0xffff:
                v = coff[j] << 16 | w
                q += [(M.VOFF, v, v), (M.VOFF, coff[0] << 16, v), (M.VOFF, v, coff[-1] << 16)]
        q.append((M.VOFF, (coff[j] + 1) << 16, (coff[j] + 1) << 16))
    for _ in range(200):
        ub = rnd.randrange(uoff[0], U + 1)
        ue = rnd.randrange(ub, U + 1)
        q.append((M.VOFF, M.voff(coff, uoff, ub), M.voff(coff, uoff, ue, at_end=rnd.random() < 0.5)))
    q.append((M.VOFF, M.voff(coff, uoff, U), M.voff(coff, uoff, uoff[0])))     # begin after end
    return q


def test_range_mapping_equals_the_model(host):
    rnd = random.Random(11)
    cases = []
    for t in range(40):
        L = rnd.choice([0, 1, 2, 3, 7, 50, 300])
        base = (rnd.randrange(0, 1 << 30), rnd.randrange(0, 1 << 33)) if t % 3 == 2 else (0, 0)   # an index slice
        coff, uoff = random_index(rnd, L, *base)
        cases.append((coff, uoff, queries(rnd, coff, uoff)))
    # an index of empty members only, and one of a single member
    cases.append(([0, 28, 56], [0, 0, 0], [(M.UOFF, 0, 0), (M.UOFF, 0, 1), (M.VOFF, 28 << 16, 56 << 16), (M.VOFF, 0, 1)]))
    cases.append(([0, 1000], [0, 65536], [(M.UOFF, 0, 65536), (M.VOFF, 0, 65536), (M.VOFF, 0, 1000 << 16), (M.VOFF, 65535, 1000 << 16 | 1)]))
    got = host(cases)
    seen = set()
    for (coff, uoff, qs), out in zip(cases, got):
        for q, g in zip(qs, out):
            want = M.resolve(coff, uoff, *q)
            assert g == want, (q, coff[:8], uoff[:8])
            seen.add(want[0])
            if want[0] == M.OK and want[3] >= 0:
                # the first and last member hold the range's first and last byte and are not empty
                assert uoff[want[3]] <= want[1] < uoff[want[3] + 1] and uoff[want[4]] <= want[2] - 1 < uoff[want[4] + 1]
    assert seen == {M.OK, M.OUT_OF_BOUNDS, M.BAD_VOFFSET}


# ---- .gzi --------------------------------------------------------------------------------------------------------------------
SINK = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t)


@pytest.fixture(scope="module")
def lib():
    L = C.CDLL(LIB)
    L.nxz_gzi_write.argtypes = [C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_uint64, SINK, C.c_void_p]
    L.nxz_gzi_read.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_size_t, C.POINTER(C.c_uint64)]
    return L


def gzi_write(lib, coff, uoff):
    parts = []
    cb = SINK(lambda u, b, n: parts.append(C.string_at(b, n)) or 0)
    arr = C.c_uint64 * len(coff)
    assert lib.nxz_gzi_write(arr(*coff), arr(*uoff), len(coff), cb, None) == 0
    return b"".join(parts)


def gzi_read(lib, b, room=None):
    n = C.c_uint64()
    rc = lib.nxz_gzi_read(b, len(b), None, None, 0, C.byref(n))
    if rc:
        return rc, None
    room = n.value if room is None else room
    c, u = (C.c_uint64 * max(room, 1))(), (C.c_uint64 * max(room, 1))()
    rc = lib.nxz_gzi_read(b, len(b), c, u, room, C.byref(n))
    return rc, (list(c[:n.value]), list(u[:n.value])) if rc == 0 else n.value


def test_gzi_round_trip(lib):
    rnd = random.Random(5)
    for L in (1, 2, 3, 40, 1000):
        coff, uoff = random_index(rnd, L)
        b = gzi_write(lib, coff, uoff)
        assert b == M.gzi_bytes(coff, uoff)
        rc, got = gzi_read(lib, b)
        assert rc == 0 and got == (coff[:-1], uoff[:-1])            # the member starts: (0, 0), then the file's entries
        assert M.gzi_parse(b) == got
    # a one-member index has no entries
    assert gzi_write(lib, [0, 500], [0, 9]) == struct.pack("<Q", 0)
    assert gzi_read(lib, struct.pack("<Q", 0)) == (0, ([0], [0]))
    # written by Python: a last entry at the end marker, or at the end of the data, is accepted
    coff, uoff = [0, 900, 1800, 1828], [0, 65280, 70000, 70000]
    for last in ((1800, 70000), (1828, 70000)):
        b = struct.pack("<Q", 2) + struct.pack("<QQ", 900, 65280) + struct.pack("<QQ", *last)
        assert gzi_read(lib, b) == (0, ([0, 900, last[0]], [0, 65280, 70000]))


def test_gzi_read_rejects_bad_files(lib):
    EILSEQ, E2BIG = -84, -7
    good = M.gzi_bytes([0, 100, 200, 300, 328], [0, 10, 20, 30, 30])
    assert gzi_read(lib, good)[0] == 0
    for k in range(len(good)):                                     # every truncation
        assert gzi_read(lib, good[:k])[0] == EILSEQ, k
    assert gzi_read(lib, good + b"\0")[0] == EILSEQ                 # trailing bytes
    assert gzi_read(lib, struct.pack("<Q", 1 << 61))[0] == EILSEQ   # a count that would overflow
    for pairs in ([(200, 20), (100, 10)], [(100, 10), (100, 20)], [(100, 20), (200, 10)], [(0, 0)]):   # not increasing
        b = struct.pack("<Q", len(pairs)) + b"".join(struct.pack("<QQ", *p) for p in pairs)
        assert gzi_read(lib, b)[0] == EILSEQ, pairs
    # uncompressed offsets may repeat (empty members)
    b = struct.pack("<Q", 2) + struct.pack("<QQ", 100, 10) + struct.pack("<QQ", 128, 10)
    assert gzi_read(lib, b)[0] == 0
    assert gzi_read(lib, good, room=2) == (E2BIG, 4)
