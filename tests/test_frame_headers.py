"""The engine's zlib / gzip header parser, trailer rule and BGZF member check (power-gzip_amd/csrc/nxz_frame.h -- what the header
and trailer kernels of nxz_frame.hip and nxz_inflate_size.hip and the BGZF discovery run on the device) compiled for the host under
AddressSanitizer, every input in an allocation of exactly its length, against an independent Python reading of RFC 1950 / 1952
(tests/framing.py)."""
import gzip
import os
import random
import struct
import subprocess
import zlib

import pytest

import framing as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    exe = tmp_path_factory.mktemp("frame") / "frame_host"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize=alignment",
                    "-I", os.path.join(ROOT, "power-gzip_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "frame_host.cpp"), "-o", str(exe)], check=True)

    def run(records):
        blob = b"".join(bytes([k, fmt]) + struct.pack("<I", len(b)) + b for k, fmt, b in records)
        r = subprocess.run([str(exe)], input=blob, capture_output=True, timeout=600)
        assert r.returncode == 0, r.stderr.decode()[-4000:]
        lines = r.stdout.decode().splitlines()
        assert len(lines) == len(records) + 1
        return [int(x) for x in lines[0].split()], [[int(x) for x in ln.split()] for ln in lines[1:]]
    return run


def _check_parse(host, cases):
    """cases: (bytes, fmt); the C parser's fields equal framing.parse's"""
    _, out = host([(0, fmt, b) for b, fmt in cases])
    for (b, fmt), got in zip(cases, out):
        want = F.parse(b, fmt)
        assert dict(zip(F.FIELDS, got)) == want, (fmt, b[:40].hex(), len(b))


def test_frame_record_layout(host):
    """nxz_batch_frame_t is 52 bytes: twelve 32-bit words, then FLG XFL OS CINFO (engine.FRAME_DTYPE mirrors it)"""
    layout, _ = host([])
    assert layout == [52, 0, 4, 8, 12, 16, 20, 24, 28, 32, 36, 40, 44, 48, 49, 50, 51]


def test_zlib_headers(host):
    data = b"framed stream " * 50
    cases = []
    for level in range(10):
        for wbits in range(9, 16):
            cases.append((F.zlib_stream(data, level, wbits=wbits), F.FMT_ZLIB))
    # a preset dictionary: FDICT, the dictionary's Adler-32 as DICTID
    c = zlib.compressobj(6, zlib.DEFLATED, 15, 8, zlib.Z_DEFAULT_STRATEGY, zdict=b"framed stream dictionary")
    fdict = c.compress(data) + c.flush()
    assert fdict[1] & 0x20
    cases.append((fdict, F.FMT_ZLIB))
    # by hand: a method other than 8, CINFO 8 and 15, FCHECK wrong, each with the others right
    def hdr(cmf, flevel=2, fdict=0):
        flg = flevel << 6 | fdict << 5
        flg += 31 - (cmf * 256 + flg) % 31 if (cmf * 256 + flg) % 31 else 0
        return bytes([cmf, flg])
    for cmf in (0x77, 0x79, 0x7f, 0x87, 0xf8, 0x08, 0x18):
        cases.append((hdr(cmf) + b"\x03\x00\0\0\0\1", F.FMT_ZLIB))
    good = F.zlib_stream(data)
    for d in range(1, 31):
        cases.append((bytes([good[0], good[1] ^ d]) + good[2:], F.FMT_ZLIB))
    # every truncation point of the plain header and of an FDICT header
    for s in (good[:8], fdict[:8]):
        cases += [(s[:k], F.FMT_ZLIB) for k in range(len(s) + 1)]
    _check_parse(host, cases)
    got = {F.parse(b, f)["status"] for b, f in cases}
    assert {F.OK, F.BAD_HEADER, F.BAD_METHOD, F.NEED_DICT, F.TRUNCATED} <= got


def test_gzip_headers_every_flag_combination(host):
    rnd = random.Random(7)
    cases = []
    for flg in range(32):
        for name_len, comment_len in ((0, 0), (5, 17), (63, 64), (65, 129)):
            h = F.gzip_header(flg, mtime=rnd.getrandbits(32), xfl=rnd.getrandbits(8), os_=rnd.getrandbits(8),
                              extra=bytes(rnd.getrandbits(8) for _ in range(rnd.randrange(0, 40))),
                              name=bytes(rnd.randrange(1, 256) for _ in range(name_len)),
                              comment=bytes(rnd.randrange(1, 256) for _ in range(comment_len)))
            body = h + F.raw_deflate(b"x" * 100) + b"\0" * 8
            cases.append((body, F.FMT_GZIP))
            cases.append((body, F.FMT_AUTO))
            if name_len == 5:
                cases += [(h[:k], F.FMT_GZIP) for k in range(len(h) + 1)]        # every truncation point
    # what Python's gzip module writes (FNAME when it has a file name)
    cases.append((gzip.compress(b"hello" * 99), F.FMT_GZIP))
    _check_parse(host, cases)


def test_gzip_long_names_and_comments(host):
    """names and comments longer than 64 KiB (the device looks at 64 bytes a step), with and without FHCRC"""
    rnd = random.Random(11)
    cases = []
    for flg in (F.FNAME, F.FCOMMENT, F.FNAME | F.FCOMMENT | F.FHCRC, F.FEXTRA | F.FNAME | F.FCOMMENT | F.FHCRC):
        h = F.gzip_header(flg, extra=b"\x01" * 300, name=bytes(rnd.randrange(1, 256) for _ in range(70001)),
                          comment=bytes(rnd.randrange(1, 256) for _ in range(66000)))
        cases.append((h + b"\3\0" + b"\0" * 8, F.FMT_GZIP))
        cases += [(h[:k], F.FMT_GZIP) for k in sorted(rnd.sample(range(len(h)), 40))]
    _check_parse(host, cases)


def test_gzip_header_crc_and_reserved_bits(host):
    cases = []
    for flg in (F.FHCRC, F.FHCRC | F.FNAME, F.FHCRC | F.FEXTRA | F.FCOMMENT | F.FTEXT):
        for ok in (True, False):
            h = F.gzip_header(flg, mtime=12345, extra=b"ab", name=b"file.txt", comment=b"a comment", hcrc_ok=ok)
            cases.append((h + F.raw_deflate(b"abc") + b"\0" * 8, F.FMT_GZIP))
    for bit in (0x20, 0x40, 0x80):
        cases.append((F.gzip_header(bit) + b"\3\0" + b"\0" * 8, F.FMT_GZIP))
        cases.append((F.gzip_header(bit | F.FNAME, name=b"n") + b"\3\0" + b"\0" * 8, F.FMT_AUTO))
    g = F.gzip_header(0)
    for bad in (b"\x1e" + g[1:], g[:1] + b"\x8c" + g[2:], g[:2] + b"\x07" + g[3:]):
        cases.append((bad + b"\3\0" + b"\0" * 8, F.FMT_GZIP))
    # the wrong format asked for
    cases.append((gzip.compress(b"x"), F.FMT_ZLIB))
    cases.append((zlib.compress(b"x"), F.FMT_GZIP))
    _check_parse(host, cases)
    got = [F.parse(b, f)["status"] for b, f in cases]
    assert got[:6] == [F.OK, F.BAD_HCRC] * 3 and got[6:12] == [F.BAD_HEADER] * 6
    assert got[12:15] == [F.BAD_HEADER, F.BAD_HEADER, F.BAD_METHOD]


def test_header_crc_by_slices(host):
    """the FHCRC check's CRC-32, made of 64 slices combined by x^(8k) as the wavefront does it, equals zlib.crc32"""
    rnd = random.Random(3)
    bufs = [bytes(rnd.getrandbits(8) for _ in range(n)) for n in list(range(0, 200)) + [1000, 4095, 65536, 70001]]
    _, out = host([(2, 0, b) for b in bufs])
    assert [o[0] for o in out] == [zlib.crc32(b) for b in bufs]


def test_bgzf_member_check(host):
    rnd = random.Random(5)
    data = bytes(rnd.getrandbits(8) for _ in range(3000)) + b"abc" * 2000
    cases = [F.BGZF_EOF, F.bgzf_member(data), F.bgzf_member(b""),
             # the BC subfield after others, and before others
             F.bgzf_member(data, before=b"XY\x03\x00abc"), F.bgzf_member(data, before=b"ZZ\x00\x00", after=b"Q1\x01\x00z"),
             F.bgzf_member(data, before=b"BD\x02\x00\x07\x00" + b"B\x43\x03\x00xyz")]
    m = F.bgzf_member(data)
    bad = [m[:3] + b"\x0c" + m[4:],                                   # FLG with FNAME too
           m[:10] + b"\x05\x00" + m[12:],                             # XLEN < 6
           m[:14] + b"\x03\x00" + m[16:],                             # SLEN 3
           m[:16] + b"\x05\x00" + m[18:],                             # BSIZE smaller than header + trailer
           m[:12] + b"BD" + m[14:],                                   # no BC subfield
           m + b"trailing foreign bytes"]                             # (still a member: BSIZE says where it ends)
    cases += bad
    cases += [m[:k] for k in (0, 1, 4, 11, 12, 17, 18, 25, 26, len(m) - 1)]
    cases += [b"\x1f\x8b\x08\x04" + bytes(rnd.getrandbits(8) for _ in range(40)) for _ in range(200)]
    _, out = host([(1, 0, b) for b in cases])
    got = [o[0] for o in out]
    assert got == [F.bgzf_member_size(b) for b in cases]
    assert got[0] == 28 and all(got[1:6]) and not any(got[6:11]) and got[11] == len(m)
    assert got[12:21] == [0] * 9


# ---- the trailer rule (nxz_frame_trailer: the trailer kernels of the framed decode, compare_check on, and of the framed size query, off) ----
def _raw_result(data, deflate_len, unread_bits=0, **over):
    """the raw result of a decode that took the deflate data and unread_bits more of the source behind it"""
    r = {"cc": F.CC_OK, "sfbt": F.SFBT_FINAL_EOB, "spbc": deflate_len + unread_bits // 8, "subc": unread_bits, "tpbc": len(data) & 0xffffffff,
         "crc": zlib.crc32(data), "adler": zlib.adler32(data)}
    r.update(over)
    return r


def _trailer_streams():
    """(format, header length, source up to the trailer, right trailer, data)"""
    data = b"the trailer stands behind the final block " * 40
    z = F.zlib_stream(data)
    g = F.gzip_member(data, flg=F.FNAME, name=b"name.txt")
    return [(F.FMT_ZLIB, 2, z[:-4], z[-4:], data), (F.FMT_GZIP, len(F.gzip_header(F.FNAME, name=b"name.txt")), g[:-8], g[-8:], data)]


def _check_trailers(host, cases):
    """cases: (format, hdr_len, source, result); the C rule equals framing.trailer's with the comparison on and off, and the
    answer without the comparison is the answer with it except that nothing is BAD_CHECK.  Returns the answers with it on."""
    recs = []
    for fmt, hdr_len, src, r in cases:
        words = struct.pack("<8I", hdr_len, r["cc"], r["sfbt"], r["spbc"], r["subc"], r["tpbc"], r["crc"], r["adler"])
        recs += [(3, fmt | 0x80, words + src), (3, fmt, words + src)]
    _, out = host(recs)
    on = []
    for k, (fmt, hdr_len, src, r) in enumerate(cases):
        got_on, got_off = tuple(out[2 * k]), tuple(out[2 * k + 1])
        assert got_on == F.trailer(src, fmt, hdr_len, r, True), (fmt, hdr_len, len(src), r)
        assert got_off == F.trailer(src, fmt, hdr_len, r, False), (fmt, hdr_len, len(src), r)
        assert got_off[0] != F.BAD_CHECK and got_off[1:] == got_on[1:]
        if got_on[0] != F.BAD_CHECK:
            assert got_off[0] == got_on[0]
        on.append(got_on)
    return on


def test_trailer_right_and_wrong_fields(host):
    """all fields right; zlib's Adler-32 wrong; gzip's CRC-32 wrong, ISIZE wrong, both wrong (the CRC decides)"""
    (zf, zh, zs, zt, data), (gf, gh, gs, gt, _) = _trailer_streams()
    zr, gr = _raw_result(data, len(zs) - zh), _raw_result(data, len(gs) - gh)
    bad_crc, bad_isize = struct.pack("<I", zlib.crc32(data) ^ 0x10), struct.pack("<I", len(data) + 1)
    cases = [(zf, zh, zs + zt, zr), (gf, gh, gs + gt, gr),
             (zf, zh, zs + bytes([zt[0] ^ 1]) + zt[1:], zr),
             (gf, gh, gs + bad_crc + gt[4:], gr), (gf, gh, gs + gt[:4] + bad_isize, gr), (gf, gh, gs + bad_crc + bad_isize, gr),
             # bytes behind the trailer are no error
             (zf, zh, zs + zt + b"more", zr), (gf, gh, gs + gt + gs, gr)]
    on = _check_trailers(host, cases)
    assert [o[0] for o in on] == [F.OK, F.OK, F.BAD_CHECK, F.BAD_CHECK, F.BAD_LENGTH, F.BAD_CHECK, F.OK, F.OK]
    assert on[0] == (F.OK, len(zs) + 4, zlib.adler32(data), 0) and on[1] == (F.OK, len(gs) + 8, zlib.crc32(data), len(data))
    assert on[5][2:] == (zlib.crc32(data) ^ 0x10, len(data) + 1)          # (reported as read)


def test_trailer_cut_at_every_length(host):
    """the source ends anywhere from the end of the deflate data to one byte short of the trailer: TRUNCATED, nothing reported"""
    cases = []
    for fmt, hdr_len, body, t, data in _trailer_streams():
        r = _raw_result(data, len(body) - hdr_len)
        cases += [(fmt, hdr_len, body + t[:k], r) for k in range(len(t))]
    on = _check_trailers(host, cases)
    assert len(on) == 4 + 8 and all(o == (F.TRUNCATED, 0, 0, 0) for o in on)


def test_trailer_behind_unread_source_bits(host):
    """a route that took more of the source than the deflate data: subc unread bits, the whole bytes among them lie behind dend"""
    cases = []
    for fmt, hdr_len, body, t, data in _trailer_streams():
        for subc in (0, 7, 8, 16, 0xfff8):
            tail = t + b"\xa5" * max(0, subc // 8 - len(t))               # (the source holds the spbc bytes the route took)
            cases.append((fmt, hdr_len, body + tail, _raw_result(data, len(body) - hdr_len, subc)))
            cases.append((fmt, hdr_len, body + t[:-1], _raw_result(data, len(body) - hdr_len, subc)))
    on = _check_trailers(host, cases)
    for (fmt, hdr_len, src, r), o in zip(cases[::2], on[::2]):
        assert o[0] == F.OK and o[1] == hdr_len + r["spbc"] - (r["subc"] >> 3) + (8 if fmt == F.FMT_GZIP else 4)
    assert all(o == (F.TRUNCATED, 0, 0, 0) for o in on[1::2])


def test_trailer_of_failed_and_unfinished_results(host):
    """no final end-of-block: the decoder's "source ran out" code is TRUNCATED, every other code DEFLATE; with the final
    end-of-block seen that code goes on to the trailer, an error code does not"""
    codes = (0, 8, 13, 21, 64, 66, 67, 68, 254)
    cases = []
    for fmt, hdr_len, body, t, data in _trailer_streams():
        n = len(body) - hdr_len
        cases.append((fmt, hdr_len, body + t, _raw_result(data, n, sfbt=0, cc=F.CC_DATA_LENGTH)))
        cases += [(fmt, hdr_len, body + t, _raw_result(data, n, sfbt=0, cc=cc)) for cc in codes]
        cases.append((fmt, hdr_len, body + t, _raw_result(data, n, cc=F.CC_DATA_LENGTH)))
        cases += [(fmt, hdr_len, body + t, _raw_result(data, n, cc=cc)) for cc in codes[1:]]
        cases.append((fmt, hdr_len, body + t, _raw_result(data, n, sfbt=F.SFBT_FINAL_EOB | 2 | 0x123 << 16)))   # (other bits of sfbt do not matter)
    on = _check_trailers(host, cases)
    per = 1 + len(codes) + 1 + len(codes) - 1 + 1
    for k in (0, per):
        st = [o[0] for o in on[k:k + per]]
        assert st == [F.TRUNCATED] + [F.DEFLATE] * len(codes) + [F.OK] + [F.DEFLATE] * (len(codes) - 1) + [F.OK]
        assert all(o[1:] == (0, 0, 0) for o in on[k:k + per] if o[0] != F.OK)
