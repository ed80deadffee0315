"""The rules of nxz_batch_deflate_streams_dict (power-gzip_amd/csrc/nxz_streams_dict.h: the first block's window, where it lies in the
dictionary's device image, the six header bytes, the bound, the refusal, the launch order of a chunk) -- the code the kernels of
nxz_streams_dict.hip and the engine's host side run -- compiled for the host under AddressSanitizer and UBSan
(tests/native/streams_dict_host.cpp).  The window is held against plain Python integers and the `prev` rule of nxz_deflate_host_hist,
the header against zlib's own deflateSetDictionary output, the bound and the refusal against the plain call's rules."""
import os
import random
import subprocess
import zlib

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RAW, ZLIB, GZIP = 0, 1, 2
DICT_LENS = [0, 15, 16, 17, 4101, 32768, 40000]
HISTS = [0, 4096, 32768]


def window(hist_max):
    return min(hist_max & ~15, 32768) if hist_max <= 32768 else 32768


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    exe = tmp_path_factory.mktemp("streams_dict") / "streams_dict_host"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "power-gzip_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "streams_dict_host.cpp"), "-o", str(exe)], check=True)

    def run(lines):
        r = subprocess.run([str(exe)], input=("\n".join(lines) + "\n").encode(), capture_output=True, timeout=600)
        assert r.returncode == 0, r.stderr.decode()[-4000:]
        return r.stdout.decode().splitlines()
    return run


def test_the_first_window(host):
    cases = [(n, h) for n in DICT_LENS for h in HISTS + [15, 16, 32767, 40000]]
    out = host(["win %d %d" % c for c in cases])
    for (n, h), line in zip(cases, out):
        h0 = min(window(h), n) & ~15                        # nxz_deflate_host.cpp: min(H, prev_len) & ~15
        assert [int(x) for x in line.split()] == [h0, 32768 - h0, n - h0], (n, h)
        assert h0 % 16 == 0 and (32768 - h0) % 16 == 0
    want = {(0, 32768): 0, (15, 32768): 0, (16, 32768): 16, (17, 32768): 16, (4101, 4096): 4096, (4101, 32768): 4096, (32768, 4096): 4096,
            (32768, 32768): 32768, (40000, 4096): 4096, (40000, 32768): 32768, (40000, 0): 0}
    for (n, h), h0 in want.items():
        assert int(host(["win %d %d" % (n, h)])[0].split()[0]) == h0, (n, h)


def test_only_the_first_block_sees_the_dictionary(host):
    for h in HISTS:
        H = window(h)
        for n in DICT_LENS:
            out = host(["bwin %d %d %d" % (k, h, n) for k in (0, 1, 2, 70000)])
            assert [int(x) for x in out] == [min(H, n) & ~15, H, H, H], (h, n)


def test_header_is_zlibs(host):
    rnd = random.Random(5)
    for d in (b"", b"a", rnd.randbytes(17), rnd.randbytes(40000)):
        for level in range(-1, 10):
            c = zlib.compressobj(level, zlib.DEFLATED, 15, 8, zlib.Z_DEFAULT_STRATEGY, d) if d else None
            if c is not None:
                want = (c.compress(b"x") + c.flush())[:6]
            else:
                # zlib takes no empty dictionary: FDICT and DICTID 1 on the header zlib writes for this level
                plain = zlib.compressobj(level).flush()[:2]
                flg = (plain[1] & 0xc0) | 0x20
                flg += 31 - (0x7800 + flg) % 31
                want = bytes([0x78, flg, 0, 0, 0, 1])
            assert want[2:] == zlib.adler32(d).to_bytes(4, "big")
            assert host(["hdr %d %d %d" % (ZLIB, level, zlib.adler32(d))])[0] == "6 " + want.hex(), (len(d), level)
            assert host(["hdr %d %d %d" % (RAW, level, zlib.adler32(d))])[0] == "0 -"


def test_formats(host):
    assert host(["fmt %d" % f for f in (RAW, ZLIB, GZIP, 3)]) == ["1", "1", "0", "0"]


def test_bound_is_the_plain_calls_plus_the_dictid(host):
    for h in HISTS:
        B = 65536 - window(h)
        for n in (0, 1, 16, B - 1, B, B + 1, 3 * B + 5, 2 ** 32 + 70000):
            raw = n + ((n + B - 1) // B) * 10 + 16
            assert host(["bound %d %d %d" % (n, h, RAW)])[0] == "%d %d" % (raw, raw)
            assert host(["bound %d %d %d" % (n, h, ZLIB)])[0] == "%d %d" % (raw + 6 + 4, raw + 6)


def test_refusals(host):
    ok = 4096
    for h in HISTS:
        for fmt, extra in ((RAW, 0), (ZLIB, 10)):
            bound = 1000 + 10 + 16 + extra
            cases = [((ok, ok, 1000, bound), 0), ((ok, ok, 1000, bound - 1), 13), ((ok + 8, ok, 1000, bound), 8), ((0, ok, 1000, bound), 8),
                     ((ok, 0, 1000, bound), 8), ((0, ok + 1, 0, 16 + extra), 0), ((ok, ok + 3, 0, 16 + extra - 1), 13)]
            out = host(["refuse %d %d %d %d %d %d" % (c + (h, fmt)) for c, _ in cases])
            assert [int(x) for x in out] == [w for _, w in cases], (h, fmt)


def test_launch_order_puts_first_blocks_in_front(host):
    rnd = random.Random(9)
    batches = [[1], [3], [0, 0, 2, 0], [1, 1, 1, 1, 1], [5, 0, 1, 7, 0, 0, 2, 1], [rnd.choice([0, 1, 1, 2, 9]) for _ in range(200)]]
    for blocks in batches:
        total = sum(blocks)
        is_first = []
        for b in blocks:
            is_first += [True] + [False] * (b - 1) if b else []
        for C in (1, 2, 3, 7, 64, total):
            out = host(["order %d %s" % (C, " ".join(map(str, blocks)))])
            assert len(out) == (total + C - 1) // C
            for c, line in enumerate(out):
                nums = [int(x) for x in line.split()]
                nf, pos = nums[0], nums[1:]
                kind = is_first[c * C:c * C + len(pos)]
                assert nf == sum(kind) and sorted(pos) == list(range(len(pos))), (blocks, C, c)
                # first blocks in front in the batch's order, the rest behind in the batch's order
                assert [p for p, f in zip(pos, kind) if f] == list(range(nf)), (blocks, C, c)
                assert [p for p, f in zip(pos, kind) if not f] == list(range(nf, len(pos))), (blocks, C, c)
