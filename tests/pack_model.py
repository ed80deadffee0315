"""A byte-exact model of the member packers (include/nxz_engine.h: nxz_batch_pack_gzip, nxz_batch_pack_zlib,
nxz_batch_pack_zlib_dict; kernels in power-gzip_amd/csrc/nxz_misc.hip), written from the header's words alone.  The packers are
pure functions of (jobs, results, source bytes, output bytes): so is this.

A job is given as the plain numbers and bytes the packer sees:
  length    source bytes without the history (src_len - hist_len)
  hist_len  bytes of history in front of the source at `src`
  cc, tpbc, crc, adler   the job's result
  src       the bytes at jobs[i].src: [history][source]
  dst       the bytes at jobs[i].dst, tpbc of them at least

The payload is the job's first tpbc output bytes; when the job failed or did not shrink (cc != 0 or tpbc >= length + 5) it is
the source as stored block(s).  LEN of a stored block is a 16-bit field: a source of more than 65 535 bytes goes out as two
stored blocks, 65 535 bytes and the rest, BFINAL on the second only."""
import struct

GZIP_OVERHEAD = 26       # 18-byte header with the BC subfield + CRC32 + ISIZE
ZLIB_OVERHEAD = 6        # CMF FLG + Adler-32
ZLIB_DICT_OVERHEAD = 10  # ... + DICTID


def is_stored(length, cc, tpbc):
    return cc != 0 or tpbc >= length + 5


def stored_blocks(source):
    """the stored fallback of `source` (RFC 1951 3.2.4): one final stored block, or 65 535 bytes + the rest in two"""
    def block(final, b):
        return struct.pack("<BHH", final, len(b), len(b) ^ 0xffff) + b
    if len(source) > 65535:
        return block(0, source[:65535]) + block(1, source[65535:])
    return block(1, source)


def payload(length, hist_len, cc, tpbc, src, dst):
    if is_stored(length, cc, tpbc):
        source = bytes(src[hist_len:hist_len + length])
        assert len(source) == length
        return stored_blocks(source)
    assert len(dst) >= tpbc
    return bytes(dst[:tpbc])


def payload_size(length, cc, tpbc):
    return (length + (10 if length > 65535 else 5)) if is_stored(length, cc, tpbc) else tpbc


def zlib_cmf_flg(level, fdict):
    """78 and FLG: FLEVEL as zlib's deflate.c sets it (0 for levels 0-1, 1 for 2-5, 2 for 6 and -1, 3 for 7-9), FDICT, FCHECK"""
    flevel = 2 if level < 0 or level == 6 else 0 if level < 2 else 1 if level < 6 else 3
    hdr = 0x78 << 8 | flevel << 6 | (0x20 if fdict else 0)
    hdr += 31 - hdr % 31
    return struct.pack(">H", hdr)


def gzip_member(length, hist_len, cc, tpbc, crc, adler, src, dst, level=-1, dictid=0):
    """ID1 ID2 CM FLG=FEXTRA MTIME=0 XFL=0 OS=255 XLEN=6 'B' 'C' SLEN=2 BSIZE = size - 1 (its low 16 bits: a member of more than
    64 KiB is valid gzip, not a BGZF member), the payload, CRC32, ISIZE"""
    p = payload(length, hist_len, cc, tpbc, src, dst)
    size = GZIP_OVERHEAD + len(p)
    head = b"\x1f\x8b\x08\x04" + bytes(4) + b"\x00\xff" + struct.pack("<H", 6) + b"BC" + struct.pack("<HH", 2, (size - 1) & 0xffff)
    return head + p + struct.pack("<II", crc, length)


def zlib_member(length, hist_len, cc, tpbc, crc, adler, src, dst, level=-1, dictid=0):
    return zlib_cmf_flg(level, False) + payload(length, hist_len, cc, tpbc, src, dst) + struct.pack(">I", adler)


def zlib_dict_member(length, hist_len, cc, tpbc, crc, adler, src, dst, level=-1, dictid=0):
    return zlib_cmf_flg(level, True) + struct.pack(">I", dictid) + payload(length, hist_len, cc, tpbc, src, dst) + struct.pack(">I", adler)


PACKERS = {"gzip": (gzip_member, GZIP_OVERHEAD), "zlib": (zlib_member, ZLIB_OVERHEAD), "zlib_dict": (zlib_dict_member, ZLIB_DICT_OVERHEAD)}


def image(packer, jobs, level=-1, dictid=0):
    """jobs: tuples (length, hist_len, cc, tpbc, crc, adler, src, dst) -> (offsets[0..n], the packed bytes)"""
    member = PACKERS[packer][0]
    offsets, parts, off = [0], [], 0
    for j in jobs:
        m = member(*j, level=level, dictid=dictid)
        parts.append(m)
        off += len(m)
        offsets.append(off)
    return offsets, b"".join(parts)


def packed_bound(packer, jobs):
    """what the header asks of `packed`: n * overhead + sum(max(tpbc, stored size of the source))"""
    over = PACKERS[packer][1]
    return sum(over + max(j[3], j[0] + (10 if j[0] > 65535 else 5)) for j in jobs)
