"""The rules of a shared preset dictionary (power-gzip_amd/csrc/nxz_dict.h: the two windows, DICTID, the zlib header with FDICT)
and the FDICT branch of the header parser (nxz_frame.h: nxz_frame_parse_dict) -- the code the device runs -- compiled for the host
under AddressSanitizer (tests/native/dict_host.cpp), against zlib itself and tests/framing.py's reading of RFC 1950."""
import os
import struct
import subprocess
import zlib

import pytest

import framing as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENS = [0, 1, 15, 16, 17, 100, 32767, 32768, 32769, 40000, 100000]
TEXT = open(os.path.join(ROOT, "tests", "golden", "alice29.txt"), "rb").read()


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    exe = tmp_path_factory.mktemp("dict") / "dict_host"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize=alignment",
                    "-I", os.path.join(ROOT, "power-gzip_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "dict_host.cpp"), "-o", str(exe)], check=True)

    def run(records):
        blob = b"".join(bytes([k, arg]) + struct.pack("<I", len(b)) + b for k, arg, b in records)
        r = subprocess.run([str(exe)], input=blob, capture_output=True, timeout=600)
        assert r.returncode == 0, r.stderr.decode()[-4000:]
        lines = r.stdout.decode().splitlines()
        assert len(lines) == len(records)
        return lines
    return run


def test_both_windows_and_dictid(host):
    out = host([(0, 0, TEXT[:n]) for n in LENS])
    for n, line in zip(LENS, out):
        iw, istart, dw, dstart, top, dictid = [int(x) for x in line.split()]
        d = TEXT[:n]
        # inflate: what zlib's inflateSetDictionary keeps -- the last min(len, 32768) bytes
        assert iw == min(n, 32768) and d[istart:] == d[n - iw:] and istart + iw == n
        # deflate: the last min(len, 32768) & ~15 bytes -- a multiple of 16, never more than the inflate window, at most 15 bytes less
        assert dw == min(n, 32768) & ~15 and dw % 16 == 0 and 0 <= iw - dw <= 15 and dstart + dw == n
        assert top == 65536 - dw
        assert dictid == zlib.adler32(d)
    assert int(host([(0, 0, b"")])[0].split()[5]) == 1


def test_the_inflate_window_is_what_zlib_keeps(host):
    """the bytes the rule picks (nxz_dict_inflate_start / _window) are all zlib looks at: a stream made with the whole dictionary
    inflates with the rule's window alone, and a stream made with the window alone inflates with the whole dictionary"""
    rec = TEXT[60000:63000] + TEXT[1000:1500] + TEXT[45000:46000]
    for n in (17, 32768, 32769, 50000, 100000):
        d = TEXT[:n]
        iw, istart = [int(x) for x in host([(0, 0, d)])[0].split()[:2]]
        window = d[istart:istart + iw]
        for made_with, read_with in ((d, window), (window, d)):
            c = zlib.compressobj(9, zlib.DEFLATED, -15, 8, zlib.Z_DEFAULT_STRATEGY, made_with)
            s = c.compress(rec) + c.flush()
            assert zlib.decompressobj(-15, zdict=read_with).decompress(s) == rec, n


def test_compress_job_fits(host):
    cases = []
    for n in LENS:
        W = min(n, 32768) & ~15
        for src_len, hist in [(0, 0), (1, 0), (65536 - W, 0), (65536 - W + 1, 0), (65536, 0), (0xffffffff, 0), (100, 16), (0, 1)]:
            cases.append((W, src_len, hist))
    out = host([(2, 0, struct.pack("<III", *c)) for c in cases])
    for (W, src_len, hist), line in zip(cases, out):
        assert int(line) == (1 if hist == 0 and W + src_len <= 65536 else 0), (W, src_len, hist)


def test_header_bytes_equal_zlibs_for_every_level(host):
    want_flg = {-1: 0xbb, 0: 0x3f, 1: 0x3f, 2: 0x7d, 3: 0x7d, 4: 0x7d, 5: 0x7d, 6: 0xbb, 7: 0xf9, 8: 0xf9, 9: 0xf9}
    for d in (b"a", TEXT[:100], TEXT[:40000]):
        out = host([(1, level + 1, d) for level in range(-1, 10)])
        for level, line in zip(range(-1, 10), out):
            c = zlib.compressobj(level, zlib.DEFLATED, 15, 8, zlib.Z_DEFAULT_STRATEGY, d)
            z = c.compress(b"some data") + c.flush()
            assert bytes.fromhex(line) == z[:6], (level, line, z[:6].hex())
            assert z[0] == 0x78 and z[1] == want_flg[level] and z[2:6] == struct.pack(">I", zlib.adler32(d))
    # an empty dictionary: zlib itself writes no FDICT; the engine does, with DICTID 1, and zlib reads that
    for level, line in zip(range(-1, 10), host([(1, level + 1, b"") for level in range(-1, 10)])):
        h = bytes.fromhex(line)
        assert h == bytes([0x78, want_flg[level], 0, 0, 0, 1]) and (h[0] * 256 + h[1]) % 31 == 0
        body = zlib.compress(b"some data", 6)[2:]
        assert zlib.decompressobj(zdict=b"").decompress(h + body) == b"some data"


def _parse_dict(host, stream, fmt, have, dictid):
    line = host([(3, fmt | (16 if have else 0), struct.pack("<I", dictid) + stream)])[0]
    return dict(zip(("status", "format", "hdr_len", "flg", "cinfo", "dictid", "use_dict"), [int(x) for x in line.split()]))


def test_fdict_branch_of_the_header_parser(host):
    d = TEXT[:5000]
    c = zlib.compressobj(6, zlib.DEFLATED, 15, 8, zlib.Z_DEFAULT_STRATEGY, d)
    fdict = c.compress(TEXT[6000:7000]) + c.flush()
    plain = zlib.compress(TEXT[6000:7000], 6)
    gz = F.gzip_member(TEXT[6000:7000], 6)
    did = zlib.adler32(d)
    model = F.parse(fdict, F.FMT_ZLIB)
    assert model["status"] == F.NEED_DICT and model["dictid"] == did and model["hdr_len"] == 6
    # the dictionary's id: decoded with it, six header bytes
    for fmt in (F.FMT_ZLIB, F.FMT_AUTO):
        got = _parse_dict(host, fdict, fmt, True, did)
        assert got == dict(status=F.OK, format=F.FMT_ZLIB, hdr_len=6, flg=model["flg"], cinfo=model["cinfo"], dictid=did, use_dict=1)
    # another id, or no dictionary given: as the model (and the plain parser) says
    for have, other in ((True, did ^ 1), (True, 1), (False, did), (False, 0)):
        got = _parse_dict(host, fdict, F.FMT_ZLIB, have, other)
        assert got["status"] == F.NEED_DICT and got["use_dict"] == 0 and got["dictid"] == did and got["hdr_len"] == 6
    # no FDICT, gzip: never with the dictionary
    for s, fmt in ((plain, F.FMT_ZLIB), (plain, F.FMT_AUTO), (gz, F.FMT_GZIP), (gz, F.FMT_AUTO)):
        got = _parse_dict(host, s, fmt, True, did)
        want = F.parse(s, fmt)
        assert got["use_dict"] == 0 and all(got[k] == want[k] for k in ("status", "format", "hdr_len", "flg", "cinfo", "dictid")), (fmt, got, want)
    # every truncation point of the FDICT header, with the right id
    for n in range(0, 8):
        got = _parse_dict(host, fdict[:n], F.FMT_ZLIB, True, did)
        want = F.parse(fdict[:n], F.FMT_ZLIB)
        if want["status"] == F.NEED_DICT:
            assert got["status"] == F.OK and got["use_dict"] == 1 and n >= 6
        else:
            assert got["status"] == want["status"] == F.TRUNCATED and got["use_dict"] == 0 and n < 6, (n, got, want)
    # a damaged FCHECK / method with FDICT set is a header fault, not a dictionary question
    bad = bytes([fdict[0], fdict[1] ^ 1]) + fdict[2:]
    assert _parse_dict(host, bad, F.FMT_ZLIB, True, did)["status"] == F.parse(bad, F.FMT_ZLIB)["status"] == F.BAD_HEADER
