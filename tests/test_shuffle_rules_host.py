"""The plan of nxz_batch_shuffle / nxz_batch_unshuffle (power-gzip_amd/csrc/nxz_shuffle.h: the tile of an element size, the tiles of a
job and their prefix, the refusals, the overlap test, what the kernel gets of a job) -- the code the engine's host side and the kernel
of nxz_shuffle.hip run -- compiled for the host under AddressSanitizer and UBSan (tests/native/shuffle_host.cpp) and held against
plain Python integers and brute force."""
import os
import random
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_OP = 8
TILE_BYTES, ELEM_MAX = 16384, 256


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    exe = tmp_path_factory.mktemp("shuffle") / "shuffle_host"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "power-gzip_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "shuffle_host.cpp"), "-o", str(exe)], check=True)

    def run(lines):
        r = subprocess.run([str(exe)], input=("\n".join(lines) + "\n").encode(), capture_output=True, timeout=600)
        assert r.returncode == 0, r.stderr.decode()[-4000:]
        return r.stdout.decode().splitlines()
    return run


def tile(elem):
    return (TILE_BYTES // elem) & ~15


def test_the_tile_of_every_element_size(host):
    out = host(["tile %d" % e for e in range(1, ELEM_MAX + 1)])
    for e, line in zip(range(1, ELEM_MAX + 1), out):
        T = int(line)
        # the most elements that fit the tile's bytes, in sixteens, and never so few that a plane's run is all head and tail
        assert T == tile(e) and T % 16 == 0 and T >= 64 and T * e <= TILE_BYTES < (T + 16) * e, e
        # ... and the planes with their shifts fit the LDS the header names
        assert e * (T + 16) <= TILE_BYTES + 16 * ELEM_MAX
        assert int(host(["slots %d" % T])[0]) == max((a + T + 15) // 16 for a in range(16))


def test_tile_counts_against_brute_force(host):
    rnd = random.Random(1)
    cases = []
    for e in (1, 2, 3, 4, 8, 16, 17, 255, 256):
        T = tile(e)
        cases += [(n, e) for n in (0, 1, T - 1, T, T + 1, 2 * T, 2 * T + 5, 10 * T - 1, rnd.randrange(0, 40 * T))]
        cases += [(2 ** 32 // e + d, e) for d in (-1, 0, 1)] + [(2 ** 32 + d, e) for d in (-1, 0, 1)]
    out = host(["tiles %d %d" % c for c in cases])
    for (n, e), line in zip(cases, out):
        T, want = tile(e), 0
        if n < 50 * 16384:
            while want * T < n:                                         # brute force: tiles until they cover the elements
                want += 1
        else:
            want = -(-n // T)
        assert int(line) == want, (n, e)


def test_overlap_of_two_ranges(host):
    a = 1 << 20
    # (a, b, len) -> overlap; ranges that touch do not overlap, empty ranges never do
    cases = [((a, a, 1), 1), ((a, a, 0), 0), ((0, 0, 0), 0), ((a, a + 100, 100), 0), ((a, a + 99, 100), 1), ((a + 100, a, 100), 0),
             ((a + 99, a, 100), 1), ((a, a + 1, 1), 0), ((a + 1, a, 1), 0), ((a, a + 1, 2), 1), ((a, a + 2 ** 32, 2 ** 32), 0),
             ((a, a + 2 ** 32 - 1, 2 ** 32), 1), ((a + 2 ** 32, a, 2 ** 32 + 1), 1), ((a, 2 ** 63, 5), 0), ((2 ** 64 - 16, 16, 8), 0)]
    out = host(["overlap %d %d %d" % c for c, _ in cases])
    assert [int(x) for x in out] == [w for _, w in cases]
    rnd = random.Random(2)
    for _ in range(300):
        x, y, n = a + rnd.randrange(0, 64), a + rnd.randrange(0, 64), rnd.randrange(0, 40)
        want = 1 if set(range(x, x + n)) & set(range(y, y + n)) else 0
        assert int(host(["overlap %d %d %d" % (x, y, n)])[0]) == want, (x, y, n)


def test_refusals(host):
    s, d = 1 << 20, 1 << 24
    # (src, dst, len, elem, reserved) -> status
    cases = [((s, d, 1000, 4, 0), 0), ((s + 1, d + 7, 1000, 3, 0), 0), ((s, d, 1000, 1, 0), 0), ((s, d, 1000, 256, 0), 0), ((s, d, 3, 256, 0), 0),
             ((0, d, 1000, 4, 0), INVALID_OP), ((s, 0, 1000, 4, 0), INVALID_OP), ((0, 0, 1000, 4, 0), INVALID_OP),
             ((0, 0, 0, 4, 0), 0), ((0, d, 0, 4, 0), 0), ((s, 0, 0, 4, 0), 0), ((s, s, 0, 4, 0), 0),
             ((s, d, 1000, 0, 0), INVALID_OP), ((s, d, 0, 0, 0), INVALID_OP), ((s, d, 1000, 257, 0), INVALID_OP), ((s, d, 1000, 2 ** 32 - 1, 0), INVALID_OP),
             ((s, d, 1000, 4, 1), INVALID_OP), ((s, d, 0, 4, 1), INVALID_OP), ((s, d, 1000, 4, 2 ** 31), INVALID_OP),
             ((s, s, 1000, 4, 0), INVALID_OP), ((s, s, 1, 1, 0), INVALID_OP), ((s, s + 999, 1000, 4, 0), INVALID_OP), ((s + 999, s, 1000, 4, 0), INVALID_OP),
             ((s, s + 1000, 1000, 4, 0), 0), ((s + 1000, s, 1000, 4, 0), 0),                    # adjacent, not overlapping
             ((s, s + 2 ** 32 + 4, 2 ** 32 + 5, 8, 0), INVALID_OP), ((s, s + 2 ** 32 + 5, 2 ** 32 + 5, 8, 0), 0)]
    out = host(["refuse %d %d %d %d %d" % c for c, _ in cases])
    assert [int(x) for x in out] == [w for _, w in cases]


def test_what_the_kernel_gets_of_a_job(host):
    s, d, far = 1 << 20, 1 << 24, 1 << 44
    # (src, dst, len, elem, reserved) -> (status, n_elems, elem, tail)
    cases = [((s, d, 10, 4, 0), (0, 2, 4, 2)), ((s, d, 7, 3, 0), (0, 2, 3, 1)), ((s, d, 12, 4, 0), (0, 3, 4, 0)),
             ((s, d, 1000, 1, 0), (0, 1000, 1, 0)), ((s, d, 3, 4, 0), (0, 3, 1, 0)), ((s, d, 255, 256, 0), (0, 255, 1, 0)),   # copies: elements of a byte
             ((s, d, 256, 256, 0), (0, 1, 256, 0)), ((s, d, 0, 4, 0), (0, 0, 1, 0)), ((0, 0, 0, 4, 0), (0, 0, 1, 0)),
             ((s, d, 1000, 0, 0), (INVALID_OP, 0, 1, 0)), ((s, s, 1000, 4, 0), (INVALID_OP, 0, 1, 0)), ((s, d, 1000, 4, 9), (INVALID_OP, 0, 1, 0)),
             ((s, far, 2 ** 32 + 7, 8, 0), (0, 2 ** 29, 8, 7)), ((s, far, 2 ** 32 - 1, 4, 0), (0, 2 ** 30 - 1, 4, 3)),
             ((s, far, 2 ** 32 + 1, 1, 0), (0, 2 ** 32 + 1, 1, 0)), ((s, far, 2 ** 40 + 3, 255, 0), (0, (2 ** 40 + 3) // 255, 255, (2 ** 40 + 3) % 255))]
    out = host(["job %d %d %d %d %d" % c for c, _ in cases])
    assert [tuple(int(x) for x in o.split()) for o in out] == [w for _, w in cases]


def test_prefix_against_brute_force(host):
    rnd = random.Random(3)
    s, d = 1 << 20, 1 << 30
    for batch in range(6):
        jobs = []
        for i in range(rnd.choice([1, 2, 7, 200])):
            elem = rnd.choice([0, 1, 2, 3, 4, 8, 16, 17, 255, 256, 300])
            n = rnd.choice([0, 1, 5, 600, 16384, 16385, 40000, 3 * 2 ** 20 + 5, 2 ** 32 + 5])
            jobs.append((s + rnd.randrange(16), d + rnd.randrange(16) if rnd.random() < 0.9 else s, n, elem, 0 if rnd.random() < 0.9 else 1))
        line = host(["batch " + " ".join("%d %d %d %d %d" % j for j in jobs)])[0]
        total, first, status = [[int(x) for x in part.split()] for part in line.split("|")]
        want_first, want_status, t = [], [], 0
        for src, dst, n, elem, reserved in jobs:
            want_first.append(t)
            bad = elem == 0 or elem > 256 or reserved or (n and set([src, dst]) & {0}) or (n and abs(src - dst) < n)
            want_status.append(INVALID_OP if bad else 0)
            if not bad:
                t += -(-n // TILE_BYTES) if elem == 1 or n < elem else -(-(n // elem) // tile(elem))
        assert total == [t] and first == want_first + [t] and status == want_status, jobs
    # 2^31 tiles and more are refused before anything is written to a grid: one job, and the sum of two
    assert host(["batch %d %d %d 1 0" % (s, 2 ** 62, 2 ** 31 * TILE_BYTES)])[0].split("|")[0].strip() == "-1"
    assert host(["batch %d %d %d 1 0" % (s, 2 ** 62, 2 ** 31 * TILE_BYTES - TILE_BYTES)])[0].split("|")[0].strip() == str(2 ** 31 - 1)
    assert host(["batch %d %d %d 1 0 %d %d %d 1 0" % (s, 2 ** 62, 2 ** 30 * TILE_BYTES, s, 2 ** 62, 2 ** 30 * TILE_BYTES)])[0].split("|")[0].strip() == "-1"
