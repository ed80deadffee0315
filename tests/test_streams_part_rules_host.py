"""The rules of nxz_batch_deflate_streams_part (power-gzip_amd/csrc/nxz_streams_part.h: the first block's window and whether it is
staged, the framing a part carries, the bound, the refusals, the carry, the staging slots of a chunk) -- the code the kernels of
nxz_streams_part.hip and the engine's host side run -- compiled for the host under AddressSanitizer and UBSan
(tests/native/streams_part_host.cpp).  The window is held against plain Python integers and the `prev` rule of nxz_deflate_host_hist,
the framing and the carry against zlib's crc32 / adler32 over the concatenation of the parts, the bound against the plain call's,
the slots against brute force."""
import os
import random
import struct
import subprocess
import zlib

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RAW, ZLIB, GZIP = 0, 1, 2
FIRST, LAST = 1, 2
HISTS = [0, 4096, 32768]
INVALID_OP, TARGET_SPACE = 8, 13


def window(hist_max):
    return min(hist_max & ~15, 32768) if hist_max <= 32768 else 32768


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    exe = tmp_path_factory.mktemp("streams_part") / "streams_part_host"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "power-gzip_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "streams_part_host.cpp"), "-o", str(exe)], check=True)

    def run(lines):
        r = subprocess.run([str(exe)], input=("\n".join(lines) + "\n").encode(), capture_output=True, timeout=600)
        assert r.returncode == 0, r.stderr.decode()[-4000:]
        return r.stdout.decode().splitlines()
    return run


def test_the_first_window(host):
    for h in HISTS + [15, 16, 32767, 40000]:
        H = window(h)
        lens = [0, 1, 15, 16, 17, H - 16, H, H + 5, 100000] if H else [0, 1, 15, 16, 17, 100000]
        out = host(["win %d %d" % (n, h) for n in lens])
        for n, line in zip(lens, out):
            assert int(line) == min(H, n) & ~15, (n, h)                # nxz_deflate_host.cpp: min(H, prev_len) & ~15
            assert int(line) % 16 == 0
    want = {(1, 32768): 0, (15, 32768): 0, (16, 32768): 16, (17, 32768): 16, (4080, 4096): 4080, (4096, 4096): 4096, (4101, 4096): 4096,
            (100000, 4096): 4096, (100000, 32768): 32768, (32752, 32768): 32752, (100000, 0): 0, (0xffffffff, 32768): 32768}
    for (n, h), h0 in want.items():
        assert int(host(["win %d %d" % (n, h)])[0]) == h0, (n, h)


def test_only_the_first_block_sees_prev(host):
    for h in HISTS:
        H = window(h)
        for n in (0, 17, H, 100000):
            out = host(["bwin %d %d %d" % (k, h, n) for k in (0, 1, 2, 70000)])
            assert [int(x) for x in out] == [min(H, n) & ~15, H, H, H], (h, n)


def test_where_the_window_lies(host):
    src = 1 << 20
    for h in HISTS:
        H = window(h)
        for pl in (0, 1, 15, 16, 17, 4095, H, H + 5):
            h0 = min(H, pl) & ~15
            # (src, src_len, prev, prev_len): contiguous, detached at 0 / 1 / 7 / 15, no prev at all, an empty part
            cases = [((src, 1000, src - pl, pl), (1, 0)), ((src, 1000, 0 if not pl else 4096, pl), (0, 1 if h0 else 0)),
                     ((src, 1000, 4097, pl), (0, 1 if h0 else 0)), ((src, 1000, 4103, pl), (0, 1 if h0 else 0)),
                     ((src, 1000, 4111, pl), (0, 1 if h0 else 0)), ((src, 0, 4096, pl), (0, 0))]
            out = host(["staged %d %d %d %d %d" % (c + (h,)) for c, _ in cases])
            assert [tuple(int(x) for x in o.split()) for o in out] == [w for _, w in cases], (h, pl)


def test_bound_and_framing_lengths(host):
    hdr, trl = {RAW: 0, ZLIB: 2, GZIP: 10}, {RAW: 0, ZLIB: 4, GZIP: 8}
    for h in HISTS:
        B = 65536 - window(h)
        for n in (0, 1, 16, B - 1, B, B + 1, 3 * B + 5, 2 ** 32 + 70000):
            raw = n + ((n + B - 1) // B) * 10 + 16                     # nxz_deflate_host_bound_hist
            for fmt in (RAW, ZLIB, GZIP):
                for flags in (0, FIRST, LAST, FIRST | LAST):
                    hl, tl = hdr[fmt] if flags & FIRST else 0, trl[fmt] if flags & LAST else 0
                    assert host(["bound %d %d %d %d" % (n, h, fmt, flags)])[0] == "%d %d %d" % (raw + hl + tl, hl, tl), (n, h, fmt, flags)


def test_framing_bytes_per_flag_combination(host):
    parts = [b"first part, ", b"", b"the second; " * 300, b"and the last."]
    whole = b"".join(parts)
    crc, adler = zlib.crc32(whole), zlib.adler32(whole)
    z = zlib.compress(whole, 6)
    co = zlib.compressobj(6, zlib.DEFLATED, 31)
    g = co.compress(whole) + co.flush()
    for level in (-1, 1, 5, 6, 9):
        zh = zlib.compressobj(level).flush()[:2]
        for flags in (0, FIRST, LAST, FIRST | LAST):
            assert host(["frame %d %d %d %d %d %d" % (RAW, level, flags, crc, adler, len(whole))])[0] == "- -"
            got = host(["frame %d %d %d %d %d %d" % (ZLIB, level, flags, crc, adler, len(whole))])[0].split()
            assert got == [zh.hex() if flags & FIRST else "-", struct.pack(">I", adler).hex() if flags & LAST else "-"], (level, flags)
            got = host(["frame %d %d %d %d %d %d" % (GZIP, level, flags, crc, adler, len(whole))])[0].split()
            assert got == ["1f8b0800000000000403" if flags & FIRST else "-", struct.pack("<II", crc, len(whole)).hex() if flags & LAST else "-"], flags
    assert z[-4:] == struct.pack(">I", adler) and g[-8:] == struct.pack("<II", crc, len(whole)) and g[:3] == bytes.fromhex("1f8b08")
    # ISIZE is the length mod 2^32
    assert host(["frame %d -1 %d 5 6 %d" % (GZIP, LAST, 2 ** 32 + 7)])[0].split()[1] == struct.pack("<II", 5, 7).hex()


def test_refusals(host):
    ok, pv = 4096, 8192
    for h in HISTS:
        for fmt, hl, tl in ((RAW, 0, 0), (ZLIB, 2, 4), (GZIP, 10, 8)):
            def bound(flags, n=1000):
                return n + (10 if n else 0) + 16 + (hl if flags & FIRST else 0) + (tl if flags & LAST else 0)
            # (src, dst, src_len, dst_cap, prev, prev_len, flags, carry_status) -> cc
            cases = [((ok, ok, 1000, bound(3), 0, 0, 3, 0), 0), ((ok, ok, 1000, bound(3) - 1, 0, 0, 3, 0), TARGET_SPACE),
                     ((ok, ok, 1000, bound(0), pv, 500, 0, 0), 0), ((ok, ok, 1000, bound(0) - 1, pv, 500, 0, 0), TARGET_SPACE),
                     ((ok, ok, 1000, bound(2), pv, 500, 2, 0), 0), ((ok, ok, 1000, bound(2) - 1, pv, 500, 2, 0), TARGET_SPACE),
                     ((ok, ok, 1000, bound(1), 0, 0, 1, 0), 0), ((ok, ok, 1000, bound(1) - 1, 0, 0, 1, 0), TARGET_SPACE),
                     # the plain call's
                     ((ok + 8, ok, 1000, bound(3), 0, 0, 3, 0), INVALID_OP), ((0, ok, 1000, bound(3), 0, 0, 3, 0), INVALID_OP),
                     ((ok, 0, 1000, bound(3), 0, 0, 3, 0), INVALID_OP), ((0, ok + 1, 0, bound(3, 0), 0, 0, 3, 0), 0),
                     ((ok, ok + 3, 0, bound(0, 0), pv, 9, 0, 0), 0), ((ok, ok + 3, 0, bound(0, 0) - 1, pv, 9, 0, 0), TARGET_SPACE),
                     # the part's own
                     ((ok, ok, 1000, bound(0), 0, 500, 0, 0), INVALID_OP),          # prev NULL with prev_len
                     ((ok, ok, 1000, bound(0), 0, 0, 0, 0), 0),                     # prev NULL without: no window
                     ((ok, ok, 1000, bound(0), pv, 0, 0, 0), 0),
                     ((ok, ok, 1000, bound(3) + 99, 0, 0, 4, 0), INVALID_OP), ((ok, ok, 1000, bound(3) + 99, 0, 0, 7, 0), INVALID_OP),
                     ((ok, ok, 1000, bound(3) + 99, 0, 0, 0x80000001, 0), INVALID_OP),
                     ((ok, ok, 1000, bound(1), pv, 16, 1, 0), INVALID_OP), ((ok, ok, 1000, bound(3), pv, 1, 3, 0), INVALID_OP),
                     ((ok, ok, 1000, bound(0), pv, 500, 0, 1), INVALID_OP), ((ok, ok, 1000, bound(2), pv, 500, 2, 1), INVALID_OP),
                     ((ok, ok, 1000, bound(2), pv, 500, 2, 7), INVALID_OP),
                     ((ok, ok, 1000, bound(1), 0, 0, 1, 1), 0), ((ok, ok, 1000, bound(3), 0, 0, 3, 1), 0),   # FIRST: the carry is not looked at
                     # an invalid part is invalid before it is too small
                     ((ok, ok, 1000, 0, 0, 500, 0, 0), INVALID_OP), ((ok, ok, 1000, 0, pv, 500, 0, 1), INVALID_OP)]
            out = host(["refuse %d %d %d %d %d %d %d %d %d %d" % (c + (h, fmt)) for c, _ in cases])
            assert [int(x) for x in out] == [w for _, w in cases], (h, fmt)


def test_carry_follows_the_concatenation(host):
    rnd = random.Random(3)
    parts = [rnd.randbytes(n) for n in (0, 1, 15, 70000, 0, 16, 65536, 33)]
    outs = [rnd.randrange(0, 80000) for _ in parts]
    carry = (0xdeadbeef, 0x12345678, 99, 77, 5, 1)                       # whatever the record held: FIRST starts afresh
    sofar, total_out = b"", 0
    for k, (p, o) in enumerate(zip(parts, outs)):
        flags = (FIRST if k == 0 else 0) | (LAST if k == len(parts) - 1 else 0)
        sofar += p
        total_out += o
        crc, adler = zlib.crc32(sofar), zlib.adler32(sofar)
        line = host(["carry %d %d %d %d %d %d %d %d %d %d %d %d" % ((1 if flags & FIRST else 0,) + carry + (crc, adler, len(p), o, flags))])[0]
        got = tuple(int(x) for x in line.split())
        assert got[:6] == ((0, 1, 0, 0, 0, 0) if k == 0 else carry), k
        carry = got[6:]
        assert carry == (crc, adler, len(sofar), total_out, k + 1, 1 if flags & LAST else 0), k
    # total_in runs past 2^32
    line = host(["carry 0 1 2 %d %d 7 0 3 4 %d 10 0" % (2 ** 32 - 5, 2 ** 33, 100)])[0]
    assert [int(x) for x in line.split()][6:] == [3, 4, 2 ** 32 + 95, 2 ** 33 + 10, 8, 0]


def test_staging_slots_of_a_chunk(host):
    rnd = random.Random(9)
    batches = [[(1, 1)], [(0, 3)], [(1, 0), (1, 0), (1, 2), (0, 0)], [(1, 1)] * 5, [(1, 5), (0, 0), (0, 1), (1, 7), (1, 0), (0, 0), (1, 2), (1, 1)],
               [(rnd.choice([0, 1]), rnd.choice([0, 1, 1, 2, 9])) for _ in range(200)]]
    for batch in batches:
        total = sum(b for _, b in batch)
        is_staged_first = []
        for s, b in batch:
            is_staged_first += [bool(s)] + [False] * (b - 1) if b else []
        for C in (1, 2, 3, 7, 64, total):
            out = host(["plan %d %s" % (C, " ".join("%d %d" % sb for sb in batch))])
            assert len(out) == (total + C - 1) // C
            for c, line in enumerate(out):
                nums = [int(x) for x in line.split()]
                sg_b0, nst, q = nums[0], nums[1], nums[2:]
                assert sg_b0 == sum(is_staged_first[:c * C]) and nst == sum(is_staged_first[c * C:(c + 1) * C]), (batch, C, c)
                assert q == list(range(nst)) and nst <= min(C, sum(is_staged_first)), (batch, C, c)
