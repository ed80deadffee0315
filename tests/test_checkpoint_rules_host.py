"""The rules of the checkpoint calls (power-gzip_amd/csrc/nxz_checkpoint.h) -- the code the kernels of nxz_checkpoint.hip run --
compiled for the host under AddressSanitizer and UBSan (tests/native/checkpoint_host.cpp) and held against Python integers: which
block headers become checkpoints, what is stored and what is only counted, the stream's record, the arithmetic of a segment, the
validity of an index, the verdict on a decoded segment and the mapping of a range onto segments."""
import bisect
import os
import random
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WINDOW = 32768
CPS_OK, CPS_STREAM_FAILED, CPS_MORE, CPS_NO_OUTPUT, CPS_INVALID = range(5)
FRAME_OK, FRAME_TRUNCATED, FRAME_DEFLATE = 0, 5, 6
CC_OK, CC_DATA_LENGTH, CC_INVALID_OP, CC_TARGET_SPACE = 0, 3, 8, 13
RANGE_OK, RANGE_OUT_OF_BOUNDS = 0, 1


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    exe = tmp_path_factory.mktemp("cp") / "checkpoint_host"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "power-gzip_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "checkpoint_host.cpp"), "-o", str(exe)], check=True)

    def run(lines):
        r = subprocess.run([str(exe)], input=("\n".join(lines) + "\n").encode(), capture_output=True, timeout=600)
        assert r.returncode == 0, (r.returncode, r.stderr.decode()[-4000:])
        out = r.stdout.decode().splitlines()
        assert len(out) == len(lines)
        return [[int(x) for x in line.split()] for line in out]
    return run


def test_the_constants_are_the_headers():
    hdr = open(os.path.join(ROOT, "include", "nxz_engine.h")).read()
    assert "enum { NXZ_CPS_OK = 0, NXZ_CPS_STREAM_FAILED, NXZ_CPS_MORE, NXZ_CPS_NO_OUTPUT, NXZ_CPS_INVALID };" in hdr
    for name, value in (("NXZ_CC_DATA_LENGTH", CC_DATA_LENGTH), ("NXZ_CC_INVALID_OP", CC_INVALID_OP), ("NXZ_CC_TARGET_SPACE", CC_TARGET_SPACE)):
        assert re.search(r"%s\s*=\s*%d," % (name, value), hdr), name


def model_rule(span, cp_cap, us):
    count, last, stored = 0, None, []
    for u in us:
        if count == 0 or u - last >= span:
            if count < cp_cap:
                stored += [count, u]
            count += 1
            last = u
    return [count] + stored


def test_jobs_with_resume_or_history_are_refused(host):
    assert host(["job 0 0", "job 1 0", "job 0 16", "job %d 0" % (3 << 20)]) == [[1], [0], [0], [0]]


def test_checkpoint_rule(host):
    rng = random.Random(5)
    cases = [(1, 4, [0]), (1, 4, [0, 0, 0]),                      # uoff equal across empty blocks: no new checkpoint
             (1, 8, [0, 10, 10, 11]), (16384, 8, [0, 16383, 16384, 32767, 32768, 32769]),
             (16384, 2, [0, 20000, 40000, 60000]),                # counted past cp_cap
             (1 << 32, 4, [0, (1 << 32) - 1, 1 << 32, (1 << 32) + 5]),     # a span of 4 GiB: 64-bit arithmetic
             (5, 3, [7, 8, 12])]                                  # (the first header is a checkpoint whatever stands in front)
    for _ in range(200):
        n = rng.randrange(1, 40)
        us, u = [], 0
        for _ in range(n):
            us.append(u)
            u += rng.choice([0, 0, 1, 7, 100, 5000, 70000])
        cases.append((rng.choice([1, 2, 100, 16384, 65536]), rng.randrange(1, 12), us))
    got = host(["rule %d %d %d %s" % (s, c, len(us), " ".join(map(str, us))) for s, c, us in cases])
    assert got == [model_rule(s, c, us) for s, c, us in cases]


def model_summary(count, cp_cap, fmt, hdr_len, fst, cc, eob, out_len, want, have):
    if fst != FRAME_OK:
        return [CPS_STREAM_FAILED, 0, fmt, hdr_len, 0, CC_INVALID_OP, fst, 0]
    if cc or not eob:
        return [CPS_STREAM_FAILED, 0, fmt, hdr_len, 0, cc or CC_DATA_LENGTH, FRAME_DEFLATE if cc else FRAME_TRUNCATED, 0]
    st = CPS_MORE if count > cp_cap else CPS_NO_OUTPUT if (want and not have) else CPS_OK
    return [st, count, fmt, hdr_len, out_len, 0, FRAME_OK, int(st in (CPS_OK, CPS_NO_OUTPUT))]


def test_stream_record(host):
    cases = [(c, cap, fmt, hl, fst, cc, eob, ol, w, h)
             for c, cap in ((1, 1), (3, 8), (9, 8), (8, 8)) for fmt, hl in ((0, 0), (1, 2), (2, 23))
             for fst in (FRAME_OK, 1, FRAME_TRUNCATED) for cc, eob in ((0, 1), (0, 0), (CC_TARGET_SPACE, 0), (66, 0))
             for ol in (0, 200000, (1 << 32) - 1) for w, h in ((0, 0), (0, 1), (1, 0), (1, 1))]
    got = host(["summary " + " ".join(map(str, c)) for c in cases])
    assert got == [model_summary(*c) for c in cases]


def model_seg(c0, c1, u0, u1):
    in_subc = (8 - (c0 & 7)) & 7
    w = min(u0, WINDOW)
    return [c0 >> 3, (c1 + 7) >> 3, in_subc, in_subc << 20, w, u1 - u0, w + ((c1 + 7) >> 3) - (c0 >> 3)]


def test_segment_arithmetic(host):
    cases = [(80, 90, 0, 0), (16, 1000, 0, 500),                           # a header at bit 0 of a byte
             (23, 1001, 100, 900), (1007, 2000, 32767, 40000),             # at bit 7; a window shorter than 32 KiB
             (1001, 2008, 32768, 32769), (1002, 2009, 32769, 99999),
             ((1 << 35) + 3, (1 << 35) + 77, (1 << 32) - 1, (1 << 32) + 10),   # offsets around 2^32 and 2^35
             ((1 << 35) - 1, (1 << 35), (1 << 32), (1 << 32) + 1), (8 * ((1 << 32) - 1) + 7, 8 * (1 << 32), 5, 6)]
    rng = random.Random(9)
    for _ in range(300):
        c0 = rng.randrange(0, 1 << rng.choice([10, 20, 33, 36]))
        u0 = rng.randrange(0, 1 << rng.choice([4, 15, 16, 33]))
        cases.append((c0, c0 + rng.randrange(1, 1 << 24), u0, u0 + rng.randrange(0, 1 << 24)))
    got = host(["seg %d %d %d %d" % c for c in cases])
    assert got == [model_seg(*c) for c in cases]


def model_valid(src_len, cbit, uoff):
    n = len(cbit)
    if n < 2 or uoff[0] != 0:
        return 0
    L = n - 1
    for j in range(L):
        c0, c1, u0, u1 = cbit[j], cbit[j + 1], uoff[j], uoff[j + 1]
        if c1 > 8 * src_len or c1 <= c0:
            return 0
        if (u1 <= u0) if j + 1 < L else (u1 < u0):
            return 0
        if min(u0, WINDOW) + ((c1 + 7) >> 3) - (c0 >> 3) > 0xffffffff or u1 - u0 > 0xffffffff:
            return 0
    return 1


def test_index_validity(host):
    good_c, good_u = [16, 1003, 2001, 3000, 3008], [0, 700, 1400, 2100, 2100]
    cases = [(400, good_c, good_u),                                        # valid, the sentinel's uoff equal across an empty final block
             (376, good_c, good_u), (375, good_c, good_u),                 # cbit[count] == 8 * src_len; one byte short: beyond the source
             (400, [16, 2001, 1003, 3000, 3008], good_u),                  # swapped
             (400, [16, 1003, 1003, 3000, 3008], good_u),                  # cbit not strictly increasing
             (400, good_c, [0, 700, 700, 2100, 2100]),                     # uoff equal between two checkpoints
             (400, good_c, [0, 1400, 700, 2100, 2100]),                    # an index that decreases
             (400, good_c, [0, 700, 1400, 2100, 2099]),                    # the sentinel below the last checkpoint
             (400, good_c, [5, 700, 1400, 2100, 2100]),                    # uoff[0] is not 0
             (400, [16], [0]), (400, [16, 90], [0, 0]),                    # no sentinel; the empty stream
             (1 << 40, [16, 8 * (1 << 32) + 16], [0, 5]),                  # a segment whose source does not fit 32 bits
             (1 << 40, [16, 8 * ((1 << 32) - 1) + 16], [0, 5]),            # ... that just does
             (1 << 40, [16, 90, 8 * ((1 << 32) - 1) + 16], [0, 40000, 40001]),   # ... that does not with its window
             (1 << 40, [16, 1 << 20], [0, 1 << 32]), (1 << 40, [16, 1 << 20], [0, (1 << 32) - 1]),   # output of 2^32 bytes / one less
             (1 << 40, [16, 1 << 34, (1 << 35) + 3, (1 << 35) + 900], [0, (1 << 32) - 1, (1 << 32) + 50, (1 << 32) + 60]),   # around 2^32 and 2^35, valid
             (1 << 62, [16, 90], [0, 1])]                                  # 8 * src_len does not fit 64 bits
    rng = random.Random(11)
    for _ in range(200):
        n = rng.randrange(2, 9)
        c = sorted(rng.sample(range(16, 5000), n))
        u = [0] + sorted(rng.sample(range(1, 9000), n - 1))
        if rng.random() < 0.5:
            k = rng.randrange(n)
            (c if rng.random() < 0.5 else u)[k] = rng.randrange(0, 6000)
        cases.append((rng.choice([625, 700, 1000]), c, u))
    got = host(["valid %d %d %s %s" % (s, len(c), " ".join(map(str, c)), " ".join(map(str, u))) for s, c, u in cases])
    exp = [[model_valid(s, c, u) if s < (1 << 61) else 0] for s, c, u in cases]
    assert got == exp
    assert exp[0] == [1] and exp[1] == [1] and exp[2] == [0] and exp[10] == [1] and exp[12] == [1] and exp[16] == [1]
    assert sum(e[0] for e in exp) > 20 and sum(1 - e[0] for e in exp) > 20


def test_segment_verdict(host):
    cases = [(CC_OK, 100, 100), (CC_DATA_LENGTH, 100, 100), (CC_DATA_LENGTH, 99, 100), (CC_TARGET_SPACE, 100, 100), (66, 0, 0), (CC_OK, 0, 0),
             (CC_OK, 5, (1 << 32) + 5)]
    assert host(["good %d %d %d" % c for c in cases]) == [[1], [1], [0], [0], [0], [1], [0]]


def test_ranges_onto_segments(host):
    uoff = [0, 700, 1400, 2100, 2100]
    L = len(uoff) - 1
    cases = [(0, 0), (0, 1), (699, 701), (700, 700), (0, 2100), (2099, 2100), (2100, 2100), (2100, 2101), (5, 4), (1399, 1400), (1400, 1401)]

    def model(b, e):
        if b > e or b < uoff[0] or e > uoff[L]:
            return [RANGE_OUT_OF_BOUNDS, 0, 0, 0, 0]
        if b == e:
            return [RANGE_OK, b, e, 0, 0]
        return [RANGE_OK, b, e, bisect.bisect_right(uoff[:L], b) - 1, bisect.bisect_right(uoff[:L], e - 1) - 1]
    got = host(["range %d %d %d %s" % (len(uoff), b, e, " ".join(map(str, uoff))) for b, e in cases])
    assert got == [model(b, e) for b, e in cases]
    assert got[4][3:] == [0, 2] and got[5][3:] == [2, 2]             # (the empty last segment holds no byte)
