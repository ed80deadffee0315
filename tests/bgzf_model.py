"""BGZF images and their member index, in plain Python: what tests/test_bgzf_ranges_host.py and tests/test_gpu_bgzf_ranges.py
check the engine's nxz_bgzf_index / nxz_bgzf_read_ranges, nxz_bgzf_range.h and the .gzi functions against.

The rules (include/nxz_engine.h): member j holds uncompressed bytes [uoff[j], uoff[j+1]); byte u lies in the last j < L with
uoff[j] <= u; a virtual offset is coff[j] << 16 | within with within <= ISIZE of j (j == L: the end, within 0)."""
import bisect
import struct
import zlib

UOFF, VOFF = 0, 1
OK, OUT_OF_BOUNDS, BAD_VOFFSET, DAMAGED = range(4)
EOF_MARKER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def member(data, level=6, extra_before=b"", extra_after=b""):
    """one BGZF member of data: gzip header with FEXTRA holding the BC subfield (optionally between other subfields)"""
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    body = c.compress(data) + c.flush()
    xlen = len(extra_before) + 6 + len(extra_after)
    size = 12 + xlen + len(body) + 8
    assert size <= 65536
    hdr = b"\x1f\x8b\x08\x04\0\0\0\0\0\xff" + struct.pack("<H", xlen) + extra_before + b"BC" + struct.pack("<HH", 2, size - 1) + extra_after
    return hdr + body + struct.pack("<II", zlib.crc32(data), len(data) & 0xffffffff)


def member_size(b, pos):
    """nxz_bgzf_member_size at b[pos:], or 0"""
    left = len(b) - pos
    if left < 26 or b[pos:pos + 4] != b"\x1f\x8b\x08\x04":
        return 0
    xlen = struct.unpack_from("<H", b, pos + 10)[0]
    if xlen < 6 or 12 + xlen + 8 > left:
        return 0
    q = 0
    while q + 4 <= xlen:
        s = pos + 12 + q
        slen = struct.unpack_from("<H", b, s + 2)[0]
        if b[s:s + 2] == b"BC" and slen == 2 and q + 6 <= xlen:
            size = struct.unpack_from("<H", b, s + 4)[0] + 1
            return size if 12 + xlen + 8 <= size <= left else 0
        q += 4 + slen
    return 0


def index(image):
    """(coff, uoff): the members chained from 0, each list members + 1 long"""
    coff, uoff, pos, u = [], [], 0, 0
    while True:
        sz = member_size(image, pos)
        if not sz:
            break
        coff.append(pos)
        uoff.append(u)
        u += struct.unpack_from("<I", image, pos + sz - 4)[0]
        pos += sz
    coff.append(pos)
    uoff.append(u)
    return coff, uoff


MAGIC = b"\x1f\x8b\x08\x04"


def candidates(image):
    """[(position, size)]: every position at which member_size is non-zero, in order -- what the discovery's scan must find"""
    out, p = [], image.find(MAGIC)
    while p >= 0:
        sz = member_size(image, p)
        if sz:
            out.append((p, sz))
        p = image.find(MAGIC, p + 1)
    return out


class Discovery:
    """what nxz_launch_bgzf_discover / nxz_launch_bgzf_coff promise for one image at one cap and max_members (discover)"""


def discover(image, cap, max_members):
    """Everything the launcher promises, by plain loops (the successor of a candidate is looked for by walking on through the list):
      ctl          [candidates C, members L, bytes the members cover, sum of ISIZE]
      complete     C <= cap.  When it is False ONLY ctl[0] and pos / size are promised: the caller runs again with cap = C
      pos, size    of the first min(C, cap) candidates
      written      0 < L <= max_members.  When it is False offsets, jobs and coff are UNWRITTEN and ctl[3] is 0
      offsets      [0 .. L]: the running sum of ISIZE (64-bit)
      members      per member (src offset, src_len, dst offset, dst_cap)
      coff         [0 .. L]: where member j starts; coff[L] = the bytes covered"""
    d = Discovery()
    cand = candidates(image)
    C = len(cand)
    d.complete = C <= cap
    d.pos = [p for p, _ in cand[:cap]]
    d.size = [s for _, s in cand[:cap]]
    chain, k = [], 0
    if cand and cand[0][0] == 0:
        chain.append(0)
        while True:
            want = cand[k][0] + cand[k][1]
            n = k + 1
            while n < C and cand[n][0] != want:                      # a linear walk
                n += 1
            if n == C:
                break
            chain.append(n)
            k = n
    L = len(chain)
    used = cand[chain[-1]][0] + cand[chain[-1]][1] if L else 0
    isz = [struct.unpack_from("<I", image, cand[k][0] + cand[k][1] - 4)[0] for k in chain]
    d.written = 0 < L <= max_members
    d.offsets, d.members, d.coff = [], [], []
    if d.written:
        o = 0
        for k, n in zip(chain, isz):
            d.offsets.append(o)
            d.members.append((cand[k][0], cand[k][1], o, n))
            d.coff.append(cand[k][0])
            o += n
        d.offsets.append(o)
        d.coff.append(used)
    d.ctl = [C, L, used, d.offsets[-1] if d.written else 0]
    d.L, d.used, d.chain = L, used, chain
    return d


def voff_to_uoff(coff, uoff, v):
    L = len(coff) - 1
    c, w = v >> 16, v & 0xffff
    k = bisect.bisect_right(coff, c)
    if k == 0 or coff[k - 1] != c:
        return None
    j = k - 1
    isize = uoff[j + 1] - uoff[j] if j < L else 0
    return uoff[j] + w if w <= isize else None


def resolve(coff, uoff, kind, b, e):
    """(status, ub, ue, first, last): first = last = -1 for a range without bytes"""
    L = len(coff) - 1
    if kind == VOFF:
        b, e = voff_to_uoff(coff, uoff, b), voff_to_uoff(coff, uoff, e)
        if b is None or e is None:
            return BAD_VOFFSET, 0, 0, -1, -1
    if b > e or b < uoff[0] or e > uoff[L]:
        return OUT_OF_BOUNDS, 0, 0, -1, -1
    if b == e:
        return OK, b, e, -1, -1
    return OK, b, e, bisect.bisect_right(uoff, b, 0, L) - 1, bisect.bisect_right(uoff, e - 1, 0, L) - 1


def voff(coff, uoff, u, at_end=False):
    """a virtual offset for uncompressed offset u (at_end: in the member that ENDS at u, within == its ISIZE, when there is one)"""
    L = len(coff) - 1
    if at_end:
        j = bisect.bisect_left(uoff, u, 0, L + 1)        # first j with uoff[j] >= u: the member before ends there
        if 0 < j <= L and uoff[j] == u and uoff[j - 1] < u:
            return coff[j - 1] << 16 | (u - uoff[j - 1])
    j = bisect.bisect_right(uoff, u, 0, L) - 1 if u < uoff[L] else L
    return coff[j] << 16 | (u - uoff[j])


def gzi_bytes(coff, uoff):
    """the .gzi of an index: the starts of members 1 .. L - 1"""
    pairs = list(zip(coff[1:-1], uoff[1:-1]))
    return struct.pack("<Q", len(pairs)) + b"".join(struct.pack("<QQ", c, u) for c, u in pairs)


def gzi_parse(b):
    (k,) = struct.unpack_from("<Q", b, 0)
    assert len(b) == 8 + 16 * k
    e = [struct.unpack_from("<QQ", b, 8 + 16 * j) for j in range(k)]
    return [0] + [c for c, _ in e], [0] + [u for _, u in e]
