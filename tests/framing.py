"""zlib (RFC 1950) / gzip (RFC 1952) / BGZF framing written out in Python, independently of the engine's parser
(power-gzip_amd/csrc/nxz_frame.h): the tests build headers with it and hold the engine's view of them against it."""
import struct
import zlib

FMT_ZLIB, FMT_GZIP, FMT_AUTO = 1, 2, 3
OK, BAD_HEADER, BAD_METHOD, NEED_DICT, BAD_HCRC, TRUNCATED, DEFLATE, BAD_CHECK, BAD_LENGTH = range(9)
FTEXT, FHCRC, FEXTRA, FNAME, FCOMMENT = 1, 2, 4, 8, 16
FIELDS = ("status", "format", "hdr_len", "extra_off", "extra_len", "name_off", "comment_off", "flg", "xfl", "os", "cinfo",
          "mtime", "dictid")


def gzip_header(flg=0, mtime=0, xfl=0, os_=255, extra=b"", name=b"", comment=b"", hcrc_ok=True):
    """a gzip header with the optional fields FLG asks for (FHCRC: right, or off by one when hcrc_ok is False)"""
    h = bytearray(b"\x1f\x8b\x08" + bytes([flg]) + struct.pack("<I", mtime) + bytes([xfl, os_]))
    if flg & FEXTRA:
        h += struct.pack("<H", len(extra)) + extra
    if flg & FNAME:
        h += name + b"\0"
    if flg & FCOMMENT:
        h += comment + b"\0"
    if flg & FHCRC:
        c = zlib.crc32(bytes(h)) & 0xffff
        h += struct.pack("<H", c if hcrc_ok else c ^ 1)
    return bytes(h)


def gzip_member(data, level=6, **hdr):
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    return gzip_header(**hdr) + c.compress(data) + c.flush() + struct.pack("<II", zlib.crc32(data), len(data) & 0xffffffff)


def raw_deflate(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
    return c.compress(data) + c.flush()


def zlib_stream(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, wbits=15):
    c = zlib.compressobj(level, zlib.DEFLATED, wbits, 8, strategy)
    return c.compress(data) + c.flush()


def parse(b, fmt):
    """the header as RFC 1950 / 1952 and zlib's order of checks read it; a field past the end is TRUNCATED"""
    n = len(b)
    f = dict.fromkeys(FIELDS, 0)
    gz = fmt == FMT_GZIP or (fmt == FMT_AUTO and n >= 2 and b[0] == 0x1f and b[1] == 0x8b)
    f["format"] = FMT_GZIP if gz else FMT_ZLIB

    def done(st):
        f["status"] = st
        return f
    if not gz:
        if n < 2:
            return done(TRUNCATED)
        cmf, flg = b[0], b[1]
        f["flg"], f["cinfo"] = flg, cmf >> 4
        if (cmf * 256 + flg) % 31:
            return done(BAD_HEADER)
        if cmf & 15 != 8:
            return done(BAD_METHOD)
        if cmf >> 4 > 7:
            return done(BAD_HEADER)
        if flg & 0x20:
            if n < 6:
                return done(TRUNCATED)
            f["dictid"], f["hdr_len"] = struct.unpack(">I", b[2:6])[0], 6
            return done(NEED_DICT)
        f["hdr_len"] = 2
        return done(OK)
    for i, want in enumerate((0x1f, 0x8b)):
        if n <= i:
            return done(TRUNCATED)
        if b[i] != want:
            return done(BAD_HEADER)
    if n < 3:
        return done(TRUNCATED)
    if b[2] != 8:
        return done(BAD_METHOD)
    if n < 4:
        return done(TRUNCATED)
    flg = f["flg"] = b[3]
    if flg & 0xe0:
        return done(BAD_HEADER)
    if n < 10:
        return done(TRUNCATED)
    f["mtime"], f["xfl"], f["os"] = struct.unpack("<I", b[4:8])[0], b[8], b[9]
    q = 10
    if flg & FEXTRA:
        if n < q + 2:
            return done(TRUNCATED)
        f["extra_len"] = struct.unpack("<H", b[q:q + 2])[0]
        f["extra_off"] = q + 2
        q += 2 + f["extra_len"]
        if q > n:
            return done(TRUNCATED)
    for bit, key in ((FNAME, "name_off"), (FCOMMENT, "comment_off")):
        if flg & bit:
            f[key] = q
            z = b.find(b"\0", q)
            if z < 0:
                return done(TRUNCATED)
            q = z + 1
    if flg & FHCRC:
        if n < q + 2:
            return done(TRUNCATED)
        if zlib.crc32(b[:q]) & 0xffff != struct.unpack("<H", b[q:q + 2])[0]:
            return done(BAD_HCRC)
        q += 2
    f["hdr_len"] = q
    return done(OK)


CC_OK, CC_DATA_LENGTH = 0, 3
SFBT_FINAL_EOB = 0x100


def trailer(src, fmt, hdr_len, res, compare_check=True):
    """(status, end, check, isize) of a framed job whose header is hdr_len bytes of format fmt and whose deflate data gave the raw
    result res (a dict of cc, sfbt, spbc, subc, tpbc, crc, adler as include/nxz_engine.h describes them).  RFC 1950: four bytes
    behind the deflate data, Adler-32 of the output, most significant byte first.  RFC 1952: eight bytes, CRC-32 of the output and
    ISIZE = its length mod 2^32, least significant byte first.  The deflate data ends where the decoder stopped: it took spbc bytes
    behind the header and left subc bits of them unprocessed, so whole unprocessed bytes belong to what follows.  Without
    compare_check the checksum is reported and not judged (a size query has no output to sum)."""
    if not res["sfbt"] & SFBT_FINAL_EOB or res["cc"] not in (CC_OK, CC_DATA_LENGTH):
        # no final end-of-block: the source ran out (the decoder's "more input" code), or the data is wrong
        return (TRUNCATED if res["cc"] == CC_DATA_LENGTH else DEFLATE), 0, 0, 0
    dend = hdr_len + res["spbc"] - res["subc"] // 8
    size = 8 if fmt == FMT_GZIP else 4
    t = src[dend:dend + size]
    if dend + size > len(src):
        return TRUNCATED, 0, 0, 0
    if fmt == FMT_GZIP:
        check, isize = struct.unpack("<II", t)
        st = BAD_CHECK if compare_check and check != res["crc"] else BAD_LENGTH if isize != res["tpbc"] else OK
    else:
        check, isize = struct.unpack(">I", t)[0], 0
        st = BAD_CHECK if compare_check and check != res["adler"] else OK
    return st, dend + size, check, isize


def bgzf_member(data, level=6, before=b"", after=b"", mtime=0):
    """one BGZF member: FLG = FEXTRA, the BC subfield (BSIZE = member size - 1) between other subfields `before` / `after`"""
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    payload = c.compress(data) + c.flush()
    xlen = len(before) + 6 + len(after)
    size = 12 + xlen + len(payload) + 8
    assert size <= 65536
    return (b"\x1f\x8b\x08\x04" + struct.pack("<I", mtime) + b"\x00\xff" + struct.pack("<H", xlen) + before +
            b"BC" + struct.pack("<HH", 2, size - 1) + after + payload + struct.pack("<II", zlib.crc32(data), len(data)))


BGZF_EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def bgzf_member_size(b, pos=0):
    """the size of the member with the BC subfield at b[pos:], or 0 (the checks of a BGZF reader)"""
    left = len(b) - pos
    p = b[pos:pos + 65536 + 32]
    if left < 26 or p[0] != 0x1f or p[1] != 0x8b or p[2] != 8 or p[3] != 4:
        return 0
    xlen = struct.unpack("<H", p[10:12])[0]
    if xlen < 6 or 12 + xlen + 8 > left:
        return 0
    q = 0
    while q + 4 <= xlen:
        si1, si2, slen = p[12 + q], p[13 + q], struct.unpack("<H", p[14 + q:16 + q])[0]
        if si1 == ord("B") and si2 == ord("C") and slen == 2 and q + 6 <= xlen:
            size = struct.unpack("<H", p[16 + q:18 + q])[0] + 1
            return size if 12 + xlen + 8 <= size <= left else 0
        q += 4 + slen
    return 0


def bgzf_scan(b):
    """members chained from position 0: (positions, bytes they cover)"""
    pos, out = 0, []
    while pos < len(b):
        s = bgzf_member_size(b, pos)
        if not s:
            break
        out.append(pos)
        pos += s
    return out, pos
