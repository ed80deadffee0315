"""The rules of the multi-member gzip calls (include/nxz_engine.h: nxz_batch_gzip_members_size / _decode) written out in Python,
independently of power-gzip_amd/csrc/nxz_gzip_members.h: headers by tests/framing.py, deflate data by zlib.  The tests hold the
engine's records and summaries against walk() / decode(), and the decoded bytes against zlib's own multi-member loop (plain())."""
import struct
import zlib

import framing as F

GZS_OK, GZS_MEMBER_FAILED, GZS_MORE_MEMBERS, GZS_TARGET_SPACE, GZS_INVALID = range(5)
MEMBER_FIELDS = ("uoff", "coff", "clen", "hdr_len", "isize", "check", "status")
STREAM_FIELDS = ("status", "members", "failed", "consumed", "out_len")


def plain(src):
    """what a gzip reader makes of src: zlib.decompressobj(wbits=31) member after member, as long as 1f 8b follows.
    Returns (bytes, bytes of src used); raises zlib.error as zlib does."""
    out, pos = b"", 0
    while True:
        d = zlib.decompressobj(31)
        out += d.decompress(src[pos:])
        if not d.eof:
            raise zlib.error("truncated member")
        pos = len(src) - len(d.unused_data)
        if src[pos:pos + 2] != b"\x1f\x8b":
            return out, pos


def member(src, pos, uoff):
    """the record of the member at src[pos:], and the bytes it makes (None unless its deflate data ended)"""
    left = src[pos:]
    m = dict.fromkeys(MEMBER_FIELDS, 0)
    m["uoff"], m["coff"] = uoff, pos
    f = F.parse(left, F.FMT_GZIP)
    m["status"] = f["status"]
    if f["status"] != F.OK:
        return m, None
    hl = m["hdr_len"] = f["hdr_len"]
    if len(left) - hl < 8:
        m["status"] = F.TRUNCATED
        return m, None
    body = left[hl:len(left) - 8]                          # the deflate data must leave room for a trailer
    d = zlib.decompressobj(-15)
    try:
        out = d.decompress(body)
    except zlib.error:
        m["status"] = F.DEFLATE
        return m, None
    if not d.eof:
        m["status"] = F.TRUNCATED
        return m, None
    dend = hl + len(body) - len(d.unused_data)
    check, isize = struct.unpack("<II", left[dend:dend + 8])
    m["clen"], m["check"], m["isize"] = dend + 8, check, len(out)
    m["status"] = F.OK if isize == len(out) & 0xffffffff else F.BAD_LENGTH
    return m, out


def walk(src, member_cap=1 << 30, resume=0, hist_len=0):
    """(summary, records, outputs): the size call's answer for one job.  records: the stored ones (at most member_cap);
    outputs[k]: the bytes of OK member k (every member found, stored or not)"""
    s = dict.fromkeys(STREAM_FIELDS, 0)
    if resume or hist_len:
        s["status"] = GZS_INVALID
        return s, [], []
    recs, outs, pos, uoff, failed = [], [], 0, 0, False
    while True:
        m, out = member(src, pos, uoff)
        if s["members"] < member_cap:
            recs.append(m)
        s["members"] += 1
        if m["status"] != F.OK:
            s["failed"] = s["members"] - 1
            failed = True
            break
        outs.append(out)
        uoff += m["isize"]
        pos = m["coff"] + m["clen"]
        s["failed"] = s["members"]
        if len(src) - pos < 2 or src[pos:pos + 2] != b"\x1f\x8b":
            break
    s["consumed"], s["out_len"] = pos, uoff
    s["status"] = GZS_MEMBER_FAILED if failed else GZS_MORE_MEMBERS if s["members"] > member_cap else GZS_OK
    return s, recs, outs


def decode(src, summary, recs, outs, member_cap, dst_cap):
    """the decode call's answer from the size call's: (summary, records, the target's bytes as a list of (uoff, bytes))"""
    s, recs = dict(summary), [dict(m) for m in recs]
    if s["status"] not in (GZS_OK, GZS_MEMBER_FAILED, GZS_MORE_MEMBERS):
        s["status"] = GZS_INVALID
        return s, recs, []
    if s["out_len"] > dst_cap:
        s["status"] = GZS_TARGET_SPACE
        return s, recs, []
    count = min(s["failed"], member_cap)
    for m in recs[:count]:
        if m["status"] != F.OK or m["coff"] + m["clen"] > len(src) or m["uoff"] + m["isize"] > dst_cap:
            s["status"] = GZS_INVALID
            return s, recs, []
    written, decoded, first_bad = [], 0, None
    for k, m in enumerate(recs[:count]):
        if zlib.crc32(outs[k]) != m["check"]:
            m["status"] = F.BAD_CHECK
            first_bad = k if first_bad is None else first_bad
        else:
            decoded += m["isize"]
        written.append((m["uoff"], outs[k]))               # (a member with a wrong CRC is decoded all the same)
    s["out_len"] = decoded
    if first_bad is not None:
        s["status"], s["failed"] = GZS_MEMBER_FAILED, first_bad
    return s, recs, written


# ---- streams the tests share ---------------------------------------------------------------------------------------------
def gz(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, **hdr):
    """one gzip member: F.gzip_member with a strategy (Z_FIXED: fixed-code blocks; level 0: stored blocks)"""
    return (F.gzip_header(**hdr) + F.raw_deflate(data, level, strategy) + struct.pack("<II", zlib.crc32(data), len(data) & 0xffffffff))


HEADERS = [dict(), dict(flg=F.FEXTRA, extra=b"XY\x03\x00abc"), dict(flg=F.FNAME, name=b"a.txt"), dict(flg=F.FCOMMENT, comment=b"no comment"),
           dict(flg=F.FHCRC), dict(flg=F.FEXTRA | F.FNAME | F.FCOMMENT | F.FHCRC, mtime=123456789, extra=b"Q\x00\x00\x00", name=b"n" * 70,
                                  comment=b"c" * 130)]


def payload(rnd, n):
    """n bytes: text-like (matches and literals), a run, or noise"""
    kind = rnd.randrange(3)
    if kind == 0:
        words = [b"the ", b"member ", b"of ", b"a ", b"gzip ", b"file ", b"walk ", b"\n"]
        out = b"".join(rnd.choice(words) for _ in range(n // 3 + 1))
        return out[:n]
    if kind == 1:
        return bytes([rnd.randrange(256)]) * n
    return rnd.randbytes(n)


def mixed_member(rnd, k, n=None):
    """member number k of a mix: the empty member (20 bytes), stored-only, fixed-code and dynamic ones, the optional header fields in turn"""
    n = rnd.randrange(1, 3000) if n is None else n
    hdr = HEADERS[k % len(HEADERS)]
    how = k % 5
    if how == 0:
        return gz(b"")
    data = payload(rnd, n)
    if how == 1:
        return gz(data, 0, **hdr)
    if how == 2:
        return gz(data, 6, zlib.Z_FIXED, **hdr)
    return gz(data, 9 if how == 3 else 1, **hdr)
