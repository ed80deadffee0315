"""The rules of nxz_batch_inflate_streams_part (power-gzip_amd/csrc/nxz_inflate_part.h: the header's byte-wise state machine, the trailer
check, the tail and in_used rule, the refusals, the records' sizes) -- the code the kernels of nxz_inflate_part.hip and the engine's
host side run -- compiled for the host under AddressSanitizer and UBSan (tests/native/inflate_part_host.cpp).  The header is fed one
byte at a time and in random splits and held against tests/framing.py on the whole header; the trailer is split at each of its bytes;
the close is held against the rule written out in plain Python over brute-forced positions."""
import itertools
import os
import random
import struct
import subprocess
import zlib

import pytest

import framing as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RAW, ZLIB, GZIP, AUTO = 0, 1, 2, 3
HEADER, BODY, TRAILER, DONE, FAILED = range(5)
MORE, S_DONE, DST_FULL, S_FAILED = range(4)
INVALID_OP = 8
FRAME = ("status", "format", "hdr_len", "end", "check", "isize", "mtime", "dictid", "extra_off", "extra_len", "name_off", "comment_off",
         "flg", "xfl", "os", "cinfo")


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    exe = tmp_path_factory.mktemp("inflate_part") / "inflate_part_host"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "power-gzip_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "inflate_part_host.cpp"), "-o", str(exe)], check=True)

    def run(lines):
        r = subprocess.run([str(exe)], input=("\n".join(lines) + "\n").encode(), capture_output=True, timeout=600)
        assert r.returncode == 0, r.stderr.decode()[-4000:]
        return r.stdout.decode().splitlines()
    return run


def test_sizes(host):
    assert host(["sizes"])[0] == "40 704 32 288"


def splits(n, rnd):
    """piece lengths: a byte at a time, and seeded random splits with empty pieces among them"""
    yield [1] * n
    for _ in range(3):
        cuts = sorted(rnd.randrange(n + 1) for _ in range(rnd.randrange(1, 6)))
        at = [0] + cuts + [n]
        yield [b - a for a, b in zip(at, at[1:])]


def check_header(host, fmt, head, rnd, behind=b"\x4b\x4c"):
    """the header (with two bytes of whatever follows) against framing.parse on the same bytes"""
    b = head + behind
    want = F.parse(b, fmt)
    lines, cases = [], list(splits(len(b), rnd))
    for sp in cases:
        lines.append("hdr %d %s %s" % (fmt, b.hex() or "-", " ".join(map(str, sp))))
    for sp, line in zip(cases, host(lines)):
        v = [int(x) for x in line.split()]
        phase, taken, f = v[0], v[1], dict(zip(FRAME, v[2:]))
        if want["status"] == F.TRUNCATED:                              # no verdict yet: every byte was taken
            assert phase == HEADER and taken == len(b), (fmt, b.hex(), sp)
            continue
        assert phase == (BODY if want["status"] == F.OK else FAILED), (fmt, b.hex(), sp)
        for k in F.FIELDS:
            assert f[k] == want[k], (k, fmt, b.hex(), sp)
        if want["status"] == F.OK:
            assert taken == want["hdr_len"], (fmt, b.hex(), sp)


def test_gzip_headers_every_flg_combination(host):
    rnd = random.Random(1)
    for flg in range(32):
        for fmt in (GZIP, AUTO):
            check_header(host, fmt, F.gzip_header(flg=flg, mtime=0x01020304 * (flg + 1) & 0xffffffff, xfl=flg & 6, os_=3, extra=b"ab\x01\x00z", name=b"n.txt",
                                                  comment=b"comment"), rnd)
    for flg in (F.FHCRC, F.FEXTRA | F.FNAME | F.FCOMMENT | F.FHCRC):
        check_header(host, GZIP, F.gzip_header(flg=flg, extra=b"q", name=b"", comment=b"", hcrc_ok=False), rnd)      # a bad FHCRC
    # cut short anywhere: no verdict
    h = F.gzip_header(flg=31, extra=b"abcd", name=b"nm", comment=b"c")
    for k in range(len(h)):
        check_header(host, GZIP, h[:k], rnd, behind=b"")


def test_fextra_lengths(host):
    rnd = random.Random(2)
    for n in (0, 1, 65535):
        for flg in (F.FEXTRA, F.FEXTRA | F.FHCRC | F.FNAME):
            check_header(host, GZIP, F.gzip_header(flg=flg, extra=bytes(rnd.randrange(256) for _ in range(n)), name=b"x"), rnd)


def test_bad_gzip_bytes(host):
    rnd = random.Random(3)
    good = bytearray(F.gzip_header(flg=F.FNAME, name=b"a"))
    for i, v in ((0, 0x1e), (1, 0x8a), (2, 7), (2, 9), (3, 0x20), (3, 0x40), (3, 0x88)):
        b = bytearray(good)
        b[i] = v
        for fmt in (GZIP, AUTO):
            check_header(host, fmt, bytes(b), rnd)


def test_zlib_headers(host):
    rnd = random.Random(4)
    for cmf, flg in itertools.product((0x78, 0x08, 0x88, 0x79, 0x77, 0x1f, 0x00, 0xff), range(0, 256, 1)):
        if (cmf * 256 + flg) % 31 == 0 or flg in (0x9c, 0x01, 0xbb, 0x20):
            for fmt in (ZLIB, AUTO):
                check_header(host, fmt, bytes([cmf, flg]) + struct.pack(">I", 0xdeadbeef), rnd, behind=b"")
    for k in range(6):                                                 # FDICT cut short: no verdict
        check_header(host, ZLIB, (b"\x78\xbb" + struct.pack(">I", 5))[:k], rnd, behind=b"")


def test_trailer_split_at_each_byte(host):
    data = b"what the stream made" * 50
    crc, adler, n = zlib.crc32(data), zlib.adler32(data), len(data)
    cases = []
    for fmt, t in ((ZLIB, struct.pack(">I", adler)), (GZIP, struct.pack("<II", crc, n))):
        bads = [(t, F.OK)]
        b = bytearray(t); b[0] ^= 1
        bads.append((bytes(b), F.BAD_CHECK))
        if fmt == GZIP:
            b = bytearray(t); b[7] ^= 0x80
            bads.append((bytes(b), F.BAD_LENGTH))
            b = bytearray(t); b[2] ^= 4; b[5] ^= 1
            bads.append((bytes(b), F.BAD_CHECK))                        # (the check first)
        for tb, want in bads:
            for k in range(len(tb) + 1):
                cases.append((fmt, tb, [k, len(tb) - k + 3], want))      # three bytes beyond: not taken
            cases.append((fmt, tb, [0, 1, 0] + [1] * (len(tb) - 1), want))
    # ISIZE is the length mod 2^32
    cases.append((GZIP, struct.pack("<II", crc, 7), [8], F.OK, 2 ** 32 + 7))
    out = host(["trailer %d %d %d %d %s %s" % (c[0], crc, adler, c[4] if len(c) > 4 else n, (c[1] + b"xyz").hex(), " ".join(map(str, c[2]))) for c in cases])
    for c, line in zip(cases, out):
        taken, rest = line.split("|")
        phase, status, check, isize, end, tail_len = (int(x) for x in rest.split())
        assert sum(int(x) for x in taken.split()) == len(c[1]) == end, c
        assert phase == (DONE if c[3] == F.OK else FAILED) and status == c[3] and tail_len == 0, c
        assert check == (struct.unpack(">I", c[1])[0] if c[0] == ZLIB else struct.unpack("<I", c[1][:4])[0]), c
        assert isize == (0 if c[0] == ZLIB else struct.unpack("<I", c[1][4:])[0]), c


def test_a_stale_record_in_phase_trailer_takes_no_more_than_a_trailer(host):
    """a carry that was never started may say TRAILER with any tail the refusals let through (up to 288): nothing is written beyond it"""
    for fmt, tl in ((ZLIB, 4), (GZIP, 8), (RAW, 0)):
        cases = [(t, n) for t in (0, 1, tl, tl + 1, 9, 100, 288) for n in (0, 1, 7, 1000)]
        out = host(["stale %d %d %d" % (fmt, t, n) for t, n in cases])
        for (t, n), line in zip(cases, out):
            k = min(n, max(tl - t, 0))
            assert line == "%d %d" % (k, t + k), (fmt, t, n)


def test_refusals(host):
    ok = 4096
    # (src, dst, prev, src_len, dst_cap, prev_len, flags, phase, tail_len) -> cc
    cases = [((ok, ok, 0, 10, 10, 0, 1, 0, 0), 0), ((ok, ok, ok, 10, 10, 5, 0, BODY, 0), 0), ((0, ok, 0, 0, 10, 0, 1, 0, 0), 0),
             ((ok, 0, 0, 10, 0, 0, 1, 0, 0), 0), ((ok, ok, 0, 10, 10, 0, 0, HEADER, 0), 0), ((ok, ok, 0, 10, 10, 0, 0, TRAILER, 7), 0),
             ((0, ok, 0, 1, 10, 0, 1, 0, 0), INVALID_OP), ((ok, 0, 0, 10, 1, 0, 1, 0, 0), INVALID_OP), ((ok, ok, 0, 10, 10, 1, 0, BODY, 0), INVALID_OP),
             ((ok, ok, 0, 10, 10, 0, 2, BODY, 0), INVALID_OP), ((ok, ok, 0, 10, 10, 0, 3, 0, 0), INVALID_OP), ((ok, ok, 0, 10, 10, 0, 0x80000001, 0, 0), INVALID_OP),
             ((ok, ok, ok, 10, 10, 16, 1, 0, 0), INVALID_OP), ((ok, ok, ok, 10, 10, 5, 0, DONE, 0), INVALID_OP), ((ok, ok, ok, 10, 10, 5, 0, FAILED, 0), INVALID_OP),
             ((ok, ok, ok, 10, 10, 5, 0, 0xa5a5a5a5, 0), INVALID_OP), ((ok, ok, ok, 10, 10, 5, 0, BODY, 289), INVALID_OP), ((ok, ok, ok, 10, 10, 5, 0, BODY, 288), 0),
             ((ok, ok, 0, 10, 10, 0, 1, DONE, 9999), 0), ((ok, ok, 0, 10, 10, 0, 1, FAILED, 0), 0)]       # FIRST: the carry is not looked at
    out = host(["refuse %d %d %d %d %d %d %d %d %d" % c for c, _ in cases])
    assert [int(x) for x in out] == [w for _, w in cases]


def close_rule(told, hist, body, src_len, spbc, subc, sfbt, tebc, cc, tpbc):
    """the tail and in_used rule in plain integers: (status, in_used, tail as (from, to) in [tail][part from body], state)"""
    L = told + src_len - body
    if cc not in (0, 3) or spbc < hist or spbc - hist > L:
        return None
    cons = spbc - hist
    back = (subc + 7) // 8
    if back > cons or (cons == L and back > 288):
        return None
    P = cons - back
    if cons == L:
        return MORE, src_len, (P, L)
    return DST_FULL, body + max(P - told, 0), (P, max(P, told))


def test_tail_and_in_used_over_brute_forced_positions(host):
    rnd = random.Random(6)
    cases = []
    for told, body, part in itertools.product((0, 1, 7, 288), (0, 3), (1, 5, 40, 400)):
        if told and body:
            continue                                                    # (a header and a tail never meet in one part)
        src_len, L = body + part, told + part
        for hist in (0, 100):
            for cons in sorted({0, 1, told, max(told - 1, 0), told + 1, L - 1, L} & set(range(L + 1))):
                for subc in (0, 1, 7, 8, 9, 15, 8 * min(cons, 287), 8 * cons, 8 * cons + 1):
                    for sfbt, tebc in ((0xa, 0), (0x9, 33), (0xc | 100 << 16, 0), (0xe, 0)):
                        cases.append((told, hist, body, src_len, 1000, hist + cons, subc, sfbt, tebc, 3, rnd.randrange(1000)))
    cases.append((0, 0, 0, 10, 1000, 10, 0, 0xa, 0, 67, 0))              # a failure
    cases.append((5, 50, 0, 10, 1000, 49, 0, 0xa, 0, 3, 0))              # fewer bytes than the window: no decode's answer
    cases.append((5, 50, 0, 10, 1000, 66, 0, 0xa, 0, 3, 0))              # more than there are
    out = host(["close " + " ".join(map(str, c)) for c in cases])
    kinds = set()
    for c, line in zip(cases, out):
        told, hist, body, src_len, cap, spbc, subc, sfbt, tebc, cc, tpbc = c
        res, car, tail = line.split("|")
        o_cc, status, in_used, out_len = (int(x) for x in res.split())
        phase, fstatus, c_sfbt, c_rem, c_subc, c_dhtlen, total_in, total_out, tail_len = (int(x) for x in car.split())
        tail = [int(x) for x in tail.split()]
        want = close_rule(told, hist, body, src_len, spbc, subc, sfbt, tebc, cc, tpbc)
        if want is None:
            assert (status, in_used, out_len, phase, fstatus, total_in, total_out) == (S_FAILED, 0, 0, FAILED, F.DEFLATE, 1000, 5000) and o_cc == cc, c
            kinds.add("failed")
            continue
        st, used, (a, b) = want
        assert (o_cc, status, in_used, out_len, phase) == (cc, st, used, tpbc, BODY), c
        assert tail_len == b - a <= 288 and tail == [k & 0xff for k in range(a, b)], c
        assert (c_sfbt, c_subc, total_in, total_out) == (sfbt & 15, subc & 7, 1000 + used, 5000 + tpbc), c
        assert c_rem == (tebc if sfbt & 0xe == 0x8 else 0) and c_dhtlen == (100 if sfbt & 0xe == 0xc else 0), c
        assert st == MORE or used < src_len, c
        kinds.add((st, used == 0 and st == DST_FULL))
    assert kinds == {"failed", (MORE, False), (DST_FULL, False), (DST_FULL, True)}


def slot_bound(prev_len, src_len):
    """nxz_inflate_part_slot_bound: the largest window, a full tail of 288 bytes, the part, rounded up to 16"""
    return (min(prev_len, 32768) + 288 + src_len + 15) & ~15


def greedy_cut(bounds, scratch, max_streams):
    """the rule in plain Python: a chunk ends in front of the stream that would carry it beyond the scratch, or at max_streams"""
    chunks, cur = [], []
    for b in bounds:
        if cur and (sum(cur) + b > scratch or len(cur) == max_streams):
            chunks.append(cur)
            cur = []
        cur.append(b)
    return chunks + [cur]


def test_the_cut_into_chunks_against_a_greedy_cut(host):
    """The engine's own cut (nxz_plan_inflate_cut, nxz_streams_plan.h) and its read-back of a chunk's stream count from off[]
    (nxz_plan_cut_streams).  The read-back ends a chunk at the next 0, so it would stop short in a chunk whose SECOND entry is 0: a
    first stream with bound 0.  nxz_inflate_part_slot_bound cannot return 0 -- it holds a full tail, 288 bytes, for any part, and adds
    in 64 bits -- so every bound here is at least 288, as every bound the engine sees is."""
    rnd = random.Random(7)
    big = 1 << 30
    cases = [("equal", 1000, 16384, [304] * 10),
             ("one larger than the scratch", 1000, 16384, [304, 5008, 304, 304]), ("the larger one first", 1000, 16384, [5008, 304]),
             ("the larger one last", 1000, 16384, [304, 5008]),
             ("exactly the scratch", 1008, 16384, [304, 304, 400]), ("one byte over", 1007, 16384, [304, 304, 400]),
             ("a single stream", 1000, 16384, [304]), ("a single stream larger than the scratch", 100, 16384, [304])]
    cases += [("max_streams %d" % k, big, k, [304] * 7) for k in (1, 2, 3)]
    for scratch in (1, 4096, 1 << 20):
        bounds = [slot_bound(rnd.choice((0, 5, 40000)), rnd.choice((0, 1, 100, 3000, 70000, 300000))) for _ in range(200)]
        cases.append(("random, scratch %d" % scratch, scratch, 16384, bounds))
        cases.append(("random, scratch %d, 5 streams" % scratch, scratch, 5, bounds))
    assert min(b for c in cases for b in c[3]) >= 288 == slot_bound(0, 0)
    out = host(["cut %d %d %s" % (scratch, most, " ".join(map(str, bounds))) for _, scratch, most, bounds in cases])
    cut_anywhere = set()
    for (name, scratch, most, bounds), line in zip(cases, out):
        *chunks, maxima = line.split(" | ")
        chunks = [[int(x) for x in ch.split()] for ch in chunks]
        want = greedy_cut(bounds, scratch, most)
        # every stream in exactly one chunk, the chunks contiguous and in order: their bounds, joined, are the batch's
        got = [[b - a for a, b in zip(ch[1:], ch[2:])] for ch in chunks]
        assert [b for g in got for b in g] == bounds, name
        assert got == want, name
        for ch, w in zip(chunks, want):
            m, off = ch[0], ch[1:]
            assert m == len(w) == len(off) - 1, name                   # the count read back from off[] is the count the cut made
            assert off[0] == 0 and off == sorted(off) and off[-1] == sum(w), name
            assert m == 1 or off[-1] <= scratch, name
            assert m <= most, name
        assert [int(x) for x in maxima.split()] == [max(len(w) for w in want), max(sum(w) for w in want)], name
        cut_anywhere.add(len(want) > 1)
    # what the named cases are there for, worked out by hand: 304 x 3 a chunk; 304 | 5008 | 304 304; no cut at 1008, one at 1007
    assert [greedy_cut(c[3], c[1], c[2]) for c in cases[1:6]] == [[[304], [5008], [304, 304]], [[5008], [304]], [[304], [5008]], [[304, 304, 400]],
                                                                  [[304, 304], [400]]]
    assert [[len(w) for w in greedy_cut(c[3], c[1], c[2])] for c in (cases[0], *cases[8:11])] == [[3, 3, 3, 1], [1] * 7, [2, 2, 2, 1], [3, 3, 1]]
    assert cut_anywhere == {False, True}
