"""What the block search of the one-stream inflate (power-gzip_amd/csrc/nxz_blockfind.hip: find_blocks_kernel,
check_headers_kernel) must answer, in plain Python: the header rule as the comment at the top of that file and RFC 1951
3.2.7 state it -- bits read one by one, code lengths kept as lists, Kraft sums as integers in units of 2^-15 -- and none of the kernel's
packed arithmetic.  No GPU, no engine.

A bit position passes (header(...).ok) when
  BTYPE is 10 (BFINAL either way), HLIT <= 29 and HDIST <= 29,
  the code-length code is complete (Kraft sum exactly 1),
  the HLIT + 257 + HDIST + 1 lengths decode inside `limit`, with no repeat (16) as the first symbol and no run across the total,
  end-of-block (256) has a code, the literal/length code is complete,
  the distance code is complete, or empty, or a single code of one bit,
  and the counts are trimmed as every encoder trims them: the last code-length-code length that is sent, the last
  literal/length length and the last distance length are not zero -- unless the count is the smallest there is (HCLEN 4,
  HLIT 257, HDIST 1) -- or the header carries the signature 286 / 30 / 19 of the table generator, which never trims.

expected(src, first_bit, seg_bytes) is what nxz_launch_find_blocks documents for `first`: per segment the lowest passer, then
the three highest passers other than that one, descending, ~0 where there is none.  It also gives K per segment (positions
that pass the 13-bit test and the code-length code's Kraft sum and whose 17 + 3 HCLEN bits fit): the kernel's caps (1024
positions kept per segment, 126 handed to the second kernel) are stated in terms of it, and npass, the number of passers."""
from collections import namedtuple

ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
NONE = (1 << 64) - 1
MORE = 3                      # NXZ_BLOCKFIND_MORE
LOOK = 320                    # bytes behind a segment that a header which starts in it may reach into
MAXCAND, LEFT_MAX = 1024, 126

# stage: 0 not BTYPE 10 / HLIT / HDIST; 1 the code-length code is not complete or does not fit; 2 the rest
Verdict = namedtuple("Verdict", "ok reason stage end")


def bits_of(src):
    """the stream as a list of bits, least significant bit of each byte first"""
    return [b >> k & 1 for b in src for k in range(8)]


ONE = 1 << 15                 # Kraft sums are integers in units of 2^-15 (no code is longer than 15 bits)


def _kraft(lens):
    return sum(ONE >> x for x in lens if x)


def _canonical(lens):
    """{(code, bits): symbol} of RFC 1951 3.2.2"""
    out, code = {}, 0
    for n in range(1, max(lens) + 1):
        for s, x in enumerate(lens):
            if x == n:
                out[(code, n)] = s
                code += 1
        code <<= 1
    return out


def header(bits, p, limit):
    """-> Verdict for a header at bit p of `bits` of which bits [0, limit) belong to the stream"""
    at = p

    class Short(Exception):
        pass

    def take(n):
        nonlocal at
        v = 0
        for k in range(n):
            if at >= limit:
                raise Short()
            v |= bits[at] << k
            at += 1
        return v

    stage = 0
    try:
        take(1)                                            # BFINAL
        if take(2) != 2:
            return Verdict(False, "btype", 0, at)
        hlit, hdist, hclen = take(5) + 257, take(5) + 1, take(4) + 4
        if hlit > 286:
            return Verdict(False, "hlit", 0, at)
        if hdist > 30:
            return Verdict(False, "hdist", 0, at)
        stage = 1
        cl = [0] * 19
        sent = []
        for s in ORDER[:hclen]:
            cl[s] = take(3)
            sent.append(cl[s])
        k = _kraft(cl)
        if k != ONE:
            return Verdict(False, "cl-over" if k > ONE else "cl-under", 1, at)
        stage = 2
        signature = (hlit, hdist, hclen) == (286, 30, 19)
        if hclen > 4 and sent[-1] == 0 and not signature:
            return Verdict(False, "trim-hclen", 2, at)
        codes = _canonical(cl)
        lens, total = [], hlit + hdist
        while len(lens) < total:
            code, n = 0, 0
            while (code, n) not in codes:
                code = code << 1 | take(1)
                n += 1
                assert n <= 7
            s = codes[(code, n)]
            if s < 16:
                run = [s]
            elif s == 16:
                if not lens:
                    return Verdict(False, "repeat-first", 2, at)
                run = [lens[-1]] * (3 + take(2))
            elif s == 17:
                run = [0] * (3 + take(3))
            else:
                run = [0] * (11 + take(7))
            if len(lens) + len(run) > total:
                return Verdict(False, "overrun", 2, at)
            lens += run
            # (a code that is over-subscribed stays so: the verdict does not depend on where it is noticed)
    except Short:
        return Verdict(False, "limit", stage, at)
    ll, dd = lens[:hlit], lens[hlit:]
    if ll[256] == 0:
        return Verdict(False, "no-256", 2, at)
    k = _kraft(ll)
    if k != ONE:
        return Verdict(False, "ll-over" if k > ONE else "ll-under", 2, at)
    k = _kraft(dd)
    nd = sum(1 for x in dd if x)
    if not (k == ONE or nd == 0 or (nd == 1 and max(dd) == 1)):
        return Verdict(False, "dist-over" if k > ONE else "dist-under", 2, at)
    if not signature:
        if hlit > 257 and ll[-1] == 0:
            return Verdict(False, "trim-hlit", 2, at)
        if hdist > 1 and dd[-1] == 0:
            return Verdict(False, "trim-hdist", 2, at)
    return Verdict(True, "ok", 2, at)


class Scan:
    """every position of a stream judged once against the whole stream; a segment's shorter `limit` then decides by where
    the header (or the part that makes it a candidate) ends: what a header reads does not depend on the limit, only whether
    it may read it"""

    def __init__(self, src):
        self.src, self.n = bytes(src), len(src)
        bits = bits_of(src)
        total = 8 * self.n
        self.v = {}                                        # position -> (Verdict, bit behind the code-length code's lengths)
        for p in range(total):
            if p + 3 > total or bits[p + 1] != 0 or bits[p + 2] != 1:
                continue
            v = header(bits, p, total)
            if v.stage == 0:
                continue
            hclen = sum(bits[p + 13 + k] << k for k in range(4)) + 4
            self.v[p] = (v, p + 17 + 3 * hclen)

    def passes(self, p, limit):
        e = self.v.get(p)
        return e is not None and e[0].ok and e[0].end <= limit

    def candidate(self, p, limit):
        """counts for K: the 13 bits and the code-length code's Kraft sum pass, and 17 + 3 HCLEN bits lie inside limit"""
        e = self.v.get(p)
        return e is not None and e[0].stage == 2 and e[1] <= limit


Expected = namedtuple("Expected", "nseg first more K npass")


def expected(src, first_bit, seg_bytes, scan=None):
    scan = scan or Scan(src)
    n = len(src)
    nseg = (n + seg_bytes - 1) // seg_bytes
    first, more, K, npass = [], [], [], []
    for g in range(nseg):
        base = g * seg_bytes
        have = min(n - base, seg_bytes + LOOK)
        limit = (base + have) * 8
        lo, hi = base * 8, base * 8 + min(have, seg_bytes) * 8
        pos = [p for p in range(max(lo, first_bit), hi) if p in scan.v]
        ok = [p for p in pos if scan.passes(p, limit)]
        K.append(sum(1 for p in pos if scan.candidate(p, limit)))
        npass.append(len(ok))
        first.append(ok[0] if ok else NONE)
        rest = sorted(ok[1:], reverse=True)[:MORE]
        more.append(rest + [NONE] * (MORE - len(rest)))
    return Expected(nseg, first, more, K, npass)


def segment_class(K, npass):
    """"two" -- the second kernel does the segment: first and more are exact; "one" -- more passers than the first kernel hands
    over, it does the segment itself: first exact, more all ~0; None -- the model cannot tell (no built case may have such a
    segment: tests/test_blockfind_model_host.py)"""
    if K > MAXCAND:
        return None
    if K <= LEFT_MAX:
        return "two"
    if npass > LEFT_MAX:
        return "one"
    return None


def segment_bytes(srclen):
    """nxz_blockfind_segment at its default setting"""
    return 1024 if srclen <= 1 << 20 else 2048 if srclen <= 2 << 20 else 4096 if srclen <= 8 << 20 else 8192
