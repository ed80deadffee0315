"""The rules of nxz_batch_deflate_streams (power-gzip_amd/csrc/nxz_streams.h: the block plan, the bound, the framing bytes and
the two checksum joins) -- the code the kernels of nxz_streams.hip run -- compiled for the host under AddressSanitizer and UBSan
(tests/native/streams_host.cpp).  The plan is held against plain Python integers, the joins against zlib.crc32 / zlib.adler32,
the framing against the bytes the stream layer writes (tests/test_stream.py)."""
import os
import random
import subprocess
import zlib

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RAW, ZLIB, GZIP = 0, 1, 2
HISTS = [0, 15, 16, 4096, 32767, 32768, 40000]


def window(hist_max):
    return min(hist_max & ~15, 32768) if hist_max <= 32768 else 32768


def sizes(B):
    return [0, 1, 15, 16, B - 1, B, B + 1, 2 * B, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 70000]


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    exe = tmp_path_factory.mktemp("streams") / "streams_host"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "power-gzip_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "streams_host.cpp"), "-o", str(exe)], check=True)

    def run(lines):
        r = subprocess.run([str(exe)], input=("\n".join(lines) + "\n").encode(), capture_output=True, timeout=600)
        assert r.returncode == 0, r.stderr.decode()[-4000:]
        return r.stdout.decode().splitlines()
    return run


def test_block_count_and_bound(host):
    cases = [(n, h) for h in HISTS for n in sizes(65536 - window(h))]
    out = host(["plan %d %d" % c for c in cases])
    assert len(out) == len(cases)
    for (n, h), line in zip(cases, out):
        H = window(h)
        B = 65536 - H
        blocks = (n + B - 1) // B
        host_bound = n + blocks * 10 + 16                  # nxz_deflate_host_bound_hist (nxz_deflate_host.cpp)
        assert [int(x) for x in line.split()] == [blocks, B, H, host_bound, host_bound + 6, host_bound + 18], (n, h)
        assert H % 16 == 0 and H <= 32768


def test_every_block_of_the_plan(host):
    for h in HISTS:
        H = window(h)
        B = 65536 - H
        for n in sizes(B):
            out = host(["blks %d %d" % (n, h)])
            blocks = (n + B - 1) // B
            assert int(out[0]) == blocks and len(out) == blocks + 1, (n, h)
            covered = 0
            for k, line in enumerate(out[1:]):
                start, length, win = line.split()
                start, length, win = int(start), int(length), int(win)
                assert (start, length, win) == (k * B, min(B, n - k * B), min(H, k * B)), (n, h, k)
                assert win % 16 == 0 and win + length <= 65536 and length > 0 and (start - win) % 16 == 0
                covered += length
            assert covered == n


def _splits(rnd, B):
    """(buffer, cut points) -- parts of length 0, 1 and exactly B among them"""
    out = []
    for _ in range(6):
        n = rnd.randrange(1, 200000)
        d = rnd.randbytes(n)
        cuts = sorted(rnd.randrange(0, n + 1) for _ in range(rnd.randrange(1, 6)))
        out.append((d, cuts))
    d = rnd.randbytes(3 * B + 1)
    out.append((d, [0, 0, 1, 1 + B, 1 + 2 * B, len(d), len(d)]))        # parts of 0, 0, 1, B, B, B, 0, 0 bytes
    out.append((b"", [0]))
    return out


def _parts(d, cuts):
    edges = [0] + list(cuts) + [len(d)]
    return [d[a:b] for a, b in zip(edges, edges[1:])]


@pytest.mark.parametrize("B", [65536, 32768, 61440])
def test_crc_join_is_zlibs(host, B):
    rnd = random.Random(B)
    for d, cuts in _splits(rnd, B):
        lines = ["reset"]
        for p in _parts(d, cuts):
            lines.append("rcrc %d %d" % (zlib.crc32(p), len(p)))
            lines.append("rcrcb %d %d %d %d" % ((zlib.crc32(p), B) + divmod(len(p), B)))
        out = host(lines)
        assert int(out[-2]) == int(out[-1]) == zlib.crc32(d), (len(d), cuts)
    # one join spelled out: crc(a + b) from crc(a), crc(b), len(b)
    a, b = rnd.randbytes(1000), rnd.randbytes(B)
    assert int(host(["crc %d %d %d" % (zlib.crc32(a), zlib.crc32(b), B)])[0]) == zlib.crc32(a + b)
    assert int(host(["crcb %d %d %d 1 0" % (zlib.crc32(a), zlib.crc32(b), B)])[0]) == zlib.crc32(a + b)


def test_crc_join_chain_of_300_parts(host):
    rnd = random.Random(300)
    parts = [rnd.randbytes(rnd.choice([0, 1, 7, 100, 4096, 65536])) for _ in range(300)]
    out = host(["reset"] + ["rcrc %d %d" % (zlib.crc32(p), len(p)) for p in parts])
    assert int(out[-1]) == zlib.crc32(b"".join(parts))
    lines = []
    # and as the layout kernel does it: every part moved over the bytes behind it, the moved values XORed
    total = sum(len(p) for p in parts)
    behind = total
    for p in parts:
        behind -= len(p)
        lines.append("crc %d 0 %d" % (zlib.crc32(p), behind))
    acc = 0
    for x in host(lines):
        acc ^= int(x)
    assert acc == zlib.crc32(b"".join(parts))


def test_adler_join_is_zlibs(host):
    rnd = random.Random(7)
    cases = _splits(rnd, 65536)
    d = rnd.randbytes(3 * 65521 + 5)
    cases.append((d, [65521, 3 * 65521, 3 * 65521]))       # parts of 65521, 2 x 65521, 0 and 5 bytes
    cases.append((b"\xff" * 200000, [1, 65521, 65522]))     # the sums at their largest
    for d, cuts in cases:
        out = host(["reset"] + ["radler %d %d" % (zlib.adler32(p), len(p)) for p in _parts(d, cuts)])
        assert int(out[-1]) == zlib.adler32(d), (len(d), cuts)
    parts = [rnd.randbytes(rnd.choice([0, 1, 100, 65521, 70000])) for _ in range(300)]
    out = host(["reset"] + ["radler %d %d" % (zlib.adler32(p), len(p)) for p in parts])
    assert int(out[-1]) == zlib.adler32(b"".join(parts))
    a, b = rnd.randbytes(1000), rnd.randbytes(2 * 65521)
    assert int(host(["adler %d %d %d" % (zlib.adler32(a), zlib.adler32(b), len(b))])[0]) == zlib.adler32(a + b)


FLG = {-1: "789c", 1: "7801", 5: "785e", 6: "789c", 9: "78da"}      # FLEVEL as nxz_batch_pack_zlib (and zlib's deflate.c) sets it


def test_header_and_trailer_bytes(host):
    for level, want in FLG.items():
        assert host(["hdr %d %d" % (ZLIB, level)])[0] == want
        assert int(want, 16) % 31 == 0
        assert host(["hdr %d %d" % (GZIP, level)])[0] == "1f8b0800000000000403"
        assert host(["hdr %d %d" % (RAW, level)])[0] == "-"
    crc, adler = 0x12345678, 0x9abcdef0
    assert host(["trl %d %d %d 5" % (RAW, crc, adler)])[0] == "-"
    assert host(["trl %d %d %d 5" % (ZLIB, crc, adler)])[0] == "9abcdef0"
    assert host(["trl %d %d %d 5" % (GZIP, crc, adler)])[0] == "78563412" + "05000000"
    assert host(["trl %d %d %d %d" % (GZIP, crc, adler, 2 ** 32 + 5)])[0] == "78563412" + "05000000"      # ISIZE is src_len mod 2^32
    assert host(["trl %d %d %d %d" % (GZIP, crc, adler, 2 ** 32 - 1)])[0] == "78563412" + "ffffffff"


def test_empty_streams_are_the_stream_layers(host):
    """tests/test_stream.py::test_empty_streams_golden_bytes (the stream layer writes FLEVEL 0 at its default level: level 1 here)"""
    assert host(["empty %d 1" % ZLIB])[0] == "7801" + "010000ffff" + "00000001"
    assert host(["empty %d -1" % GZIP])[0] == "1f8b0800000000000403" + "010000ffff" + "00000000" + "00000000"
    assert host(["empty %d -1" % RAW])[0] == "010000ffff"
    for fmt, wbits in ((ZLIB, 15), (GZIP, 31), (RAW, -15)):
        for level in FLG:
            assert zlib.decompress(bytes.fromhex(host(["empty %d %d" % (fmt, level)])[0]), wbits) == b""


def test_refusals(host):
    ok = 4096
    bound = {fmt: 1000 + 10 + 16 + extra for fmt, extra in ((RAW, 0), (ZLIB, 6), (GZIP, 18))}
    for fmt in (RAW, ZLIB, GZIP):
        cases = [((ok, ok, 1000, bound[fmt]), 0), ((ok, ok, 1000, bound[fmt] - 1), 13), ((ok + 8, ok, 1000, bound[fmt]), 8),
                 ((0, ok, 1000, bound[fmt]), 8), ((ok, 0, 1000, bound[fmt]), 8), ((0, ok + 1, 0, bound[fmt]), 0),
                 ((ok, ok + 3, 0, 16 + bound[fmt] - 1026), 0), ((ok, ok, 0, 16 + bound[fmt] - 1027), 13)]
        out = host(["refuse %d %d %d %d 0 %d" % (c + (fmt,)) for c, _ in cases])
        assert [int(x) for x in out] == [w for _, w in cases], fmt
