"""Hand-built BGZF images for the member discovery (power-gzip_amd/csrc/nxz_frame.hip: bgzf_scan_kernel, tile_scan_kernel,
succ_kernel, jump_kernel, chain_kernel, member_kernel, layout_kernel, coff_kernel), each named after the edge it pins, the
same list on every call.  tests/test_bgzf_discover_sim.py runs them through the kernels on the CPU, tests/test_gpu_bgzf_discover.py
on the device; both hand what the launcher left to check() here, which holds it to tests/bgzf_model.py discover().

Payloads are stored (level 0) so that a member start can be placed to the byte.  A case lies at byte `head` of a 16-byte granule
(the scan reads whole granules: what lies in front of packed[0] and behind packed[len - 1] is `before` / `after`, 64 bytes each,
0xee where the case does not say otherwise).  decodable: every chained member is a real gzip member, so the image can go
through nxz_batch_unpack_gzip and the host's nxz_blocked_scan.  device_only: too large for the simulation.  full: the simulation
runs it with NXZ_SIM_FULL only (the device runs every case).

Edges that cannot be reached, kept on purpose:
  - head-*-header-ends-at-packed: a complete 18-byte header in front of packed[0] starts 18 bytes before it, and the scan reads
    no further back than the granule of packed[0] (head <= 15): no lane ever looks at it.  The cases that CAN be misread are
    head-*-header-at-minus-1 and head-*-header-at-granule-start, whose header starts in the granule and runs on into the image.
  - *-header-at-len: when head + len is a multiple of 16 the header behind the image lies in a granule no lane reads.
  - len < 26 is refused by the callers before the discovery runs: end-len-26 is the shortest image there is."""
import struct
import zlib

import numpy as np

import bgzf_model as M

PAD = 64                                   # bytes of `before` and of `after`
SENTINEL = 0xa5
JOB_DTYPE = np.dtype([("src", "<u8"), ("dst", "<u8"), ("src_len", "<u4"), ("hist_len", "<u4"), ("dst_cap", "<u4"), ("in_crc", "<u4"),
                      ("in_adler", "<u4"), ("dht_index", "<u4"), ("resume", "<u4"), ("reserved", "<u4")])
FAMILIES = ("head", "straddle", "end", "header-rule", "chain", "limits", "tiles")
CHAIN_L = (1, 2, 3, 4, 7, 8, 9, 15, 16, 17, 1023, 1024, 1025, 2049)


class Case:
    def __init__(self, name, image, head=3, cap=None, max_members=None, decodable=True, device_only=False, full=False,
                 before=b"", after=b""):
        assert 0 <= head < 16 and len(before) <= PAD and len(after) <= PAD
        self.name, self.family = name, next(f for f in FAMILIES if name.startswith(f + "-"))
        self.image, self.head, self.decodable, self.device_only, self.full = bytes(image), head, decodable, device_only, full
        self.before = b"\xee" * (PAD - len(before)) + before
        self.after = after + b"\xee" * (PAD - len(after))
        self._cap, self._mm, self._model = cap, max_members, None

    # (cap and max_members where the case does not set them: room for every candidate and member, and some to spare)
    @property
    def cap(self):
        return self._cap if self._cap is not None else len(M.candidates(self.image)) + 4

    @property
    def max_members(self):
        return self._mm if self._mm is not None else len(M.index(self.image)[0]) - 1 + 2

    def model(self):
        if self._model is None:
            self._model = M.discover(self.image, self.cap, self.max_members)
        return self._model


def filler(n, seed=0):
    """n bytes that never hold 1f 8b"""
    return ((np.arange(n, dtype=np.int64) * 7 + seed) % 251).astype(np.uint8).tobytes()


def header(size, extra=None, flg=4, xlen=None):
    """a gzip header with FEXTRA: the BC subfield alone says `size`, or `extra` as it stands"""
    if extra is None:
        extra = b"BC" + struct.pack("<HH", 2, size - 1)
    return b"\x1f\x8b\x08" + bytes([flg]) + b"\0\0\0\0\0\xff" + struct.pack("<H", len(extra) if xlen is None else xlen) + extra


def stored(payload, before=b"", after=b"", isize=None):
    """a member whose deflate stream is one stored block of payload: 12 + XLEN + 5 + len(payload) + 8 bytes"""
    n = len(payload)
    size = 12 + len(before) + 6 + len(after) + 5 + n + 8
    assert n <= 0xffff and size <= 65536
    extra = before + b"BC" + struct.pack("<HH", 2, size - 1) + after
    return (header(size, extra) + b"\x01" + struct.pack("<HH", n, n ^ 0xffff) + payload +
            struct.pack("<II", zlib.crc32(payload), n if isize is None else isize))


def sized(size, seed=0):
    """a stored member of exactly `size` bytes (31 .. 65536)"""
    m = stored(filler(size - 31, seed))
    assert len(m) == size
    return m


def small(j):
    return stored(filler(j % 3 + (j % 7 == 0), j))


def three():
    return stored(filler(100, 1)) + stored(b"") + stored(filler(37, 2))


def with_fakes(size, fakes, seed=0):
    """a stored member of `size` bytes whose payload holds header(fsize) at position p of the member for (p, fsize) in fakes"""
    m = bytearray(sized(size, seed))
    for p, fsize in fakes:
        assert 23 <= p and p + 18 <= size - 8
        m[p:p + 18] = header(fsize)
    pay = bytes(m[23:size - 8])
    m[size - 8:size - 4] = struct.pack("<I", zlib.crc32(pay))
    return bytes(m)


# the header forms of the family header-rule: name -> (the header of a member of `size` bytes, whether it is one)
def _rule_headers(size):
    bc = b"BC" + struct.pack("<HH", 2, size - 1)
    one, two = b"XY" + struct.pack("<H", 3) + b"abc", b"Z\x01" + struct.pack("<H", 0)
    return {
        "flg-0": (header(size, flg=0), False),
        "xlen-5": (header(size, b"BC\x02\x00" + bc[4:5], xlen=5) + bc[5:], False),
        "xlen-6": (header(size), True),
        "bc-behind-one": (header(size, one + bc), True),
        "bc-behind-two": (header(size, one + two + bc), True),
        "bc-slen-3": (header(size, b"BC" + struct.pack("<H", 3) + bc[4:] + b"q"), False),
        "bc-at-xlen-minus-5": (header(size, b"XY" + struct.pack("<H", 1) + b"q" + bc[:5]) + bc[5:], False),
        "slen-past-xlen": (header(size, b"XY" + struct.pack("<H", 20) + b"ab") + b"c" * 18 + bc, False),
        "xlen-65535": (header(size, bc, xlen=65535), False),
    }


def _head_cases():
    out = []
    for h in range(16):
        img = three()
        out.append(Case("head-%d-three-members" % h, img, head=h))
        if h in (0, 15):
            out.append(Case("head-%d-header-ends-at-packed" % h, img, head=h, before=header(26)))
        # a header that starts in front of packed[0], in its granule, and is complete only with the image's first bytes: no candidate,
        # and with no member at position 0 the true members further on are candidates that nothing chains to
        for k in sorted(k for k in {1, h} if 0 < k <= h):
            hd = header(40)
            tag = "minus-1" if k == 1 else "granule-start"
            out.append(Case("head-%d-header-at-%s" % (h, tag), hd[k:] + filler(40, h) + img, head=h, before=hd[:k], decodable=False))
        out.append(Case("head-%d-header-at-len" % h, img + filler(h % 5, 3), head=h, after=header(26) + filler(16, 4)))
        hd = header(26) + filler(8, 5)
        cut = 1 + h % 3
        out.append(Case("head-%d-header-straddles-len" % h, img + filler(7 + h, 6) + hd[:cut], head=h, after=hd[cut:]))
    return out


def _straddle_cases():
    out = []
    spots = [("granule-byte-%d" % r, 1600 + r) for r in range(16)]
    spots += [("%d-minus-%d" % (e, d), e - d) for e in (4096, 16384, 20480) for d in (3, 2, 1, 0)]
    for i, (tag, b) in enumerate(spots):
        h = (3, 0, 15, 8)[i % 4]
        p = b - h                                                          # the position that lies at byte b from the granule of packed[0]
        out.append(Case("straddle-true-" + tag, sized(p, i) + stored(filler(50, i)) + stored(filler(9, i)), head=h))
        out.append(Case("straddle-false-" + tag, with_fakes(p + 300, [(p, 26 + i)], i) + stored(filler(9, i)), head=h,
                        full=tag.startswith("granule-byte") and int(tag.split("-")[-1]) < 12))
    return out


def _end_cases():
    out, m3 = [], three()
    out.append(Case("end-last-member-ends-at-len", m3))
    out.append(Case("end-one-foreign-byte", m3 + b"\x00"))
    for g, k in ((16, 10), (4096, 1), (16384, 1)):
        for delta in (-1, 0, 1):
            n = g * k + delta - 5
            front = stored(filler(11, 1)) + stored(b"")
            out.append(Case("end-head+len-%d%+d" % (g * k, delta), front + sized(n - len(front), delta + 1), head=5))
    for d in (25, 26, 27):
        out.append(Case("end-header-%d-before-len" % d, m3 + header(26) + filler(d - 18, d), decodable=d == 25))
    for tag, size in (("left", 40), ("left+1", 41), ("least", 26), ("least-1", 25)):
        out.append(Case("end-size-%s" % tag, m3 + header(size) + filler(22, size), decodable=size in (41, 25)))
    last = stored(filler(60, 9))
    out.append(Case("end-truncated-by-1", m3 + last[:-1]))
    out.append(Case("end-truncated-to-20", m3 + last[:20]))
    out.append(Case("end-len-26", header(26) + filler(8, 1), decodable=False))
    out.append(Case("end-len-27", header(27) + filler(9, 2), decodable=False))
    out.append(Case("end-len-27-one-foreign", header(26) + filler(9, 3), decodable=False))
    out.append(Case("end-len-28-the-end-marker", M.EOF_MARKER))
    return out


def _rule_cases():
    out = []
    a, tail = stored(filler(64, 1)), stored(filler(5, 2))
    for name in _rule_headers(26):
        big = name == "xlen-65535"                                         # (its XLEN fits only an image of more than 64 KiB behind it)
        # in a payload: the size leads to the next true member
        size = 4000 - 200
        hd = _rule_headers(size)[name][0]
        m = bytearray(sized(4000, 3))
        m[200:200 + len(hd)] = hd
        m[-8:-4] = struct.pack("<I", zlib.crc32(bytes(m[23:-8])))
        img = bytes(m) + tail + (sized(65536, 4) + sized(200, 5) if big else b"")
        out.append(Case("header-rule-%s-in-a-payload" % name, img, full=big))
        # as the would-be second member: a real member where the header is one, else bytes that nothing chains to
        hd, ok = _rule_headers(31)[name]
        if ok:
            second = stored(b"", before=hd[12:len(hd) - 6])
            assert second[:len(hd)] == _rule_headers(len(second))[name][0]
        else:
            second = hd + filler(31, 6)
        out.append(Case("header-rule-%s-as-second-member" % name, a + second + tail + (sized(65536, 4) + sized(200, 5) if big else b""), full=big))
    return out


def _chain_cases():
    out, m3 = [], three()
    out.append(Case("chain-candidate-0-at-position-1", b"\x00" + m3, decodable=False))
    b, c = stored(filler(20, 1)), stored(filler(3, 2))
    out.append(Case("chain-false-leads-to-a-true-start", with_fakes(500, [(123, 500 - 123)]) + b + c))
    out.append(Case("chain-false-leads-nowhere", with_fakes(500, [(123, 100)]) + b + c))
    out.append(Case("chain-false-leads-to-a-false-one", with_fakes(500, [(123, 100), (223, 50)]) + b + c))
    out.append(Case("chain-false-run-rejoins-two-members-on", with_fakes(500, [(123, 100), (223, 500 - 223 + len(b))]) + b + c + stored(b"z")))
    for L in CHAIN_L:
        img = b"".join(small(j) for j in range(L))
        for cap in (L, L + 1):
            out.append(Case("chain-%d-members-cap-%d" % (L, cap), img, cap=cap, max_members=L, full=L > 17))
    return out


def second_pass_image():
    """four true members, the first a stored payload of 60 KiB with a false header every 18 bytes: over 3000 candidates"""
    n = 60 * 1024
    first = with_fakes(31 + n, [(23 + 18 * k, 26) for k in range((n - 26) // 18)], 7)
    return first + stored(filler(10, 1)) + stored(b"") + stored(filler(77, 2))


def _limit_cases():
    out, m3 = [], three()
    img = with_fakes(500, [(100, 30), (200, 31), (300, 32)]) + stored(filler(5, 1))
    out.append(Case("limits-candidates-equal-cap", img, cap=5))
    out.append(Case("limits-candidates-cap-plus-1", img, cap=4))
    out.append(Case("limits-members-equal-max", m3, max_members=3))
    out.append(Case("limits-members-max-plus-1", m3, max_members=2))
    out.append(Case("limits-max-members-0", m3, max_members=0))
    two = stored(filler(9, 1), isize=0xffffffff) + stored(filler(4, 2), isize=0xffffffff)
    out.append(Case("limits-isize-ffffffff-twice", two, max_members=2, decodable=False))
    # (with two members the start of the second, 2^32 - 1, still fits 32 bits: the third member's start is the first that does not)
    out.append(Case("limits-isize-ffffffff-three-times", two + stored(b"", isize=0xffffffff), max_members=3, decodable=False))
    sp = second_pass_image()
    out.append(Case("limits-second-pass-first-cap", sp, cap=1032, max_members=4, full=True))
    out.append(Case("limits-second-pass-every-candidate", sp, max_members=4, full=True))
    return out


def _tile_image(tiles, seed):
    """stored members of 64 KiB of filler with a false header every 50 000 bytes or so, head + len one byte into the last tile"""
    n = (tiles - 1) * 16384 + 1 - 3
    out, k = [], 0
    while n:
        size = 65536 if n >= 65536 + 31 else n if n <= 65536 else n - 31
        p = 23 + (k * 7919) % 60000
        out.append(with_fakes(size, [(p, 26 + k % 40)] if p + 18 <= size - 8 else [], seed + k))
        n -= size
        k += 1
    return b"".join(out)


def _tile_cases():
    return [Case("tiles-%d" % t, _tile_image(t, t), device_only=True) for t in (1025, 2049)]


_cases = None


def cases():
    global _cases
    if _cases is None:
        _cases = _head_cases() + _straddle_cases() + _end_cases() + _rule_cases() + _chain_cases() + _limit_cases() + _tile_cases()
        names = [c.name for c in _cases]
        assert len(set(names)) == len(names)
    return _cases


def by_family():
    return {f: [c for c in cases() if c.family == f] for f in FAMILIES}


def plains(c):
    """the members' data, for a decodable case: zlib reads every chained member"""
    coff, _ = M.index(c.image)
    return [zlib.decompress(c.image[a:b], 31) for a, b in zip(coff, coff[1:])]


def check(c, got):
    """what is wrong with what the launchers left for case c, a line each.  got: ctl (4), pos, size (cap entries), offsets, coff
    (max_members + 1 entries), jobs (cap records), all numpy arrays as read back, the unwritten parts still SENTINEL; packed and
    dst, the addresses given; guards: {name: intact}"""
    m, bad = c.model(), []
    S8, S4 = int.from_bytes(bytes([SENTINEL]) * 8, "little"), int.from_bytes(bytes([SENTINEL]) * 4, "little")

    def say(what, a, b):
        bad.append("%s: %s is %s, the model says %s" % (c.name, what, a, b))

    for name, ok in got["guards"].items():
        if not ok:
            bad.append("%s: written outside %s" % (c.name, name))
    ctl = [int(x) for x in got["ctl"]]
    if ctl[0] != m.ctl[0]:
        say("ctl[0]", ctl[0], m.ctl[0])
    n = len(m.pos)
    pos, size = [int(x) for x in got["pos"][:n]], [int(x) for x in got["size"][:n]]
    if pos != m.pos or size != m.size:
        k = next((i for i in range(n) if (pos[i], size[i]) != (m.pos[i], m.size[i])), n)
        say("candidate %d of %d" % (k, n), (pos[k], size[k]) if k < n else None, (m.pos[k], m.size[k]) if k < n else None)
    if not m.complete:
        return bad                                   # (the list is cut: the caller runs again with room for ctl[0])
    if ctl != m.ctl:
        say("ctl", ctl, m.ctl)
    offsets, coff, jobs = got["offsets"], got["coff"], got["jobs"]
    L = m.L if m.written else -1
    if [int(x) for x in offsets[:L + 1]] != m.offsets:
        say("offsets", [int(x) for x in offsets[:L + 1]][:8], m.offsets[:8])
    if [int(x) for x in coff[:L + 1]] != m.coff:
        say("coff", [int(x) for x in coff[:L + 1]][:8], m.coff[:8])
    if not (offsets[L + 1:] == S8).all():
        bad.append("%s: offsets written behind [%d]" % (c.name, L))
    if not (coff[L + 1:] == S8).all():
        bad.append("%s: coff written behind [%d]" % (c.name, L))
    want = np.zeros(max(L, 0), JOB_DTYPE)
    for j, (so, sl, do, dc) in enumerate(m.members):
        want[j] = (got["packed"] + so, (got["dst"] + do) & 0xffffffffffffffff, sl, 0, dc, 0, 1, 0, 0, 0)
    if jobs[:max(L, 0)].tobytes() != want.tobytes():
        k = next(i for i in range(L) if jobs[i].tobytes() != want[i].tobytes())
        say("jobs[%d]" % k, jobs[k], want[k])
    if not (jobs[max(L, 0):].view(np.uint32) == S4).all():
        bad.append("%s: jobs written behind [%d]" % (c.name, max(L, 0)))
    return bad
