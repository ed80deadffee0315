"""DEFLATE streams written bit by bit, for the inflate routes (no GPU, no engine import): the header and symbol edges of
RFC 1951 that neither system zlib nor the project's encoder ever writes -- incomplete codes, codes of 15 bits, repeat runs
across the HLIT/HDIST boundary, length 258 as 284 + 31, empty stored blocks in the middle of a stream, one distance code or
none, forty one-symbol blocks in a row, distance 32768 exactly -- and every way such a stream can be wrong or end early.

cases() is the list [(name, stream, history)].  A name is "family/rule":
  valid/    zlib accepts the stream as well
  lenient/  the oracle accepts it and zlib rejects it: an incomplete code of which only assigned codes are used
            (oracle/nxz_huff.c refuses over-subscription only; zlib refuses the header)
  error/    the oracle's verdict is 66, 67 or 68 once the bits are there: each error in the first block with nothing
            behind it ("at-the-end"), with 8 zero bytes behind it ("padded"), and in the third block behind 30 KiB of output
            ("third-block").  A code that cannot be decoded in the last bits of the source, with fewer bits left than the
            longest code has, SUSPENDS in the oracle (zlib fails at once): the two first placements pin that rule (the
            third has the 8 bytes behind it)
  target/   the stream wants more than the capacity every case that is not valid gets (CAP_REST): 13
  cut/      valid streams cut at a byte inside HLIT/HDIST/HCLEN, inside the code-length code's lengths, inside the extra
            bits of a 16, 17 or 18, between a length's extra bits and its distance, inside LEN/NLEN

Every stream decodes to 40 KiB at the most, but for the one with a stored block of 65535 bytes, the format's longest.
HCLEN 4 is among the errors: its code-length code has the symbols 16, 17, 18 and 0 only, which cannot give the end-of-block
symbol a length; HCLEN 5 (symbol 8: 256 codes of 8 bits) is the lowest a valid stream can have.

records() adds what the CPU oracle (tests/oracle_lib.py inflate) says to each case, computed once a process: nothing here
is a pinned literal.  tests/test_deflate_handmade_host.py says what the set must hold and holds the oracle to zlib.  Rec's
fields are named as tests/resume_cases.py's Case, so that the checks of tests/test_gpu_inflate_resume.py read them.  The set
runs through the workgroup kernel on the CPU (tests/test_inflate_wg_sim.py) and through every route, the size and the verify
call on the device (tests/test_gpu_deflate_handmade.py)."""
import ctypes as C
import zlib
from collections import namedtuple

import oracle_lib as O

CAP_REST = 40 * 1024 + 64           # the capacity of every case that is not valid (valid ones: exactly their output)
ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
LBASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LEXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DBASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193,
         12289, 16385, 24577)
DEXTRA = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)
FAMILIES = ("valid", "lenient", "error", "target", "cut")
CUT_KINDS = ("hlit-hdist-hclen", "code-length-lengths", "extra-of-16", "extra-of-17", "extra-of-18", "length-and-distance", "len-nlen")

Rec = namedtuple("Rec", "name family src hist cap out err tpbc final_eob out_sfbt out_subc out_rem out_dht out_dhtlen crc1 adler1")


class Bits:
    """bits go in from the least significant bit of each byte on; Huffman codes most significant bit first (RFC 1951 3.1.1)"""

    def __init__(self):
        self.buf, self.acc, self.k = bytearray(), 0, 0
        self.regions = []                                  # (kind, first bit, bit behind): where cut/ cases cut

    @property
    def n(self):
        return 8 * len(self.buf) + self.k

    def put(self, val, nbits):
        assert 0 <= val < 1 << nbits or (nbits == 0 and val == 0), (val, nbits)
        self.acc |= val << self.k
        self.k += nbits
        while self.k >= 8:
            self.buf.append(self.acc & 0xff)
            self.acc >>= 8
            self.k -= 8

    def code(self, c, nbits):
        for i in range(nbits - 1, -1, -1):
            self.put(c >> i & 1, 1)

    def align(self):
        if self.k:
            self.put(0, 8 - self.k)

    def raw(self, data):
        assert self.k == 0
        self.buf += data

    def bits(self, data, nbits):
        """nbits bits of a bit string that is packed the same way (a table as the engine's ABI holds it)"""
        for i in range(nbits):
            self.put(data[i >> 3] >> (i & 7) & 1, 1)

    def region(self, kind, a):
        self.regions.append((kind, a, self.n))

    def data(self):
        return bytes(self.buf) + (bytes([self.acc]) if self.k else b"")


def canonical(lens):
    """{symbol: (code, bits)} of RFC 1951 3.2.2; over-subscribed lengths give codes that do not fit their bits (never written)"""
    count = [0] * 16
    for x in lens:
        count[x] += 1
    count[0] = 0
    code, nxt = 0, [0] * 16
    for b in range(1, 16):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    out = {}
    for s, x in enumerate(lens):
        if x:
            out[s] = (nxt[x], x)
            nxt[x] += 1
    return out


def kraft(lens):
    return sum(2.0 ** -x for x in lens if x)


FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DD = [5] * 32                                        # (30 and 31 have codes and no meaning)
# complete codes over every symbol: 60 x 9 + 226 x 8 bits; 2 x 4 + 28 x 5 bits; and the code-length code 13 x 4 + 6 x 5 bits
GEN_LL = [9] * 60 + [8] * 226
GEN_DD = [4] * 2 + [5] * 28
GEN_CL = [4] * 13 + [5] * 6
assert kraft(GEN_LL) == kraft(GEN_DD) == kraft(GEN_CL) == 1.0


class Coder:
    """the symbols of one block with its two codes"""

    def __init__(self, w, ll, dd):
        self.w, self.ll, self.dd = w, canonical(ll), canonical(dd)

    def sym(self, s):
        self.w.code(*self.ll[s])

    def lits(self, data):
        for b in data:
            self.w.code(*self.ll[b])

    def length(self, s, extra):
        self.w.code(*self.ll[s])
        self.w.put(extra, LEXTRA[s - 257] if s < 286 else 0)

    def dist(self, s, extra):
        self.w.code(*self.dd[s])
        self.w.put(extra, DEXTRA[s] if s < 30 else 0)

    def match(self, length, dist, lsym=None):
        """lsym: 284 for length 258 as 284 + 31"""
        ls = lsym - 257 if lsym else max(i for i in range(29) if LBASE[i] <= length)
        self.length(257 + ls, length - LBASE[ls])
        a = self.w.n
        ds = max(i for i in range(30) if DBASE[i] <= dist)
        self.dist(ds, dist - DBASE[ds])
        self.w.region("length-and-distance", a)

    def eob(self):
        self.sym(256)

    def raw(self, c, nbits):
        self.w.code(c, nbits)


def stored(w, data, final=0, nlen=None):
    w.put(final, 1); w.put(0, 2)
    w.align()
    a = w.n
    w.put(len(data), 16); w.put(len(data) ^ 0xffff if nlen is None else nlen, 16)
    w.region("len-nlen", a)
    w.raw(data)


def fixed(w, final=0):
    w.put(final, 1); w.put(1, 2)
    return Coder(w, FIXED_LL, FIXED_DD)


def plain(lens):
    return [(x, None) for x in lens]


def with_runs(lens, runs):
    """the code-length symbols of `lens` with the runs [(index, 16 | 17 | 18, entries)] written as that symbol"""
    out, i = [], 0
    runs = dict((a, (s, k)) for a, s, k in runs)
    while i < len(lens):
        if i in runs:
            s, k = runs[i]
            assert all(x == (lens[i - 1] if s == 16 else 0) for x in lens[i:i + k]) and len(lens[i:i + k]) == k
            out.append((s, k - (11 if s == 18 else 3)))
            i += k
        else:
            out.append((lens[i], None))
            i += 1
    return out


def dynamic(w, final, ll, dd, hclen=19, cl=GEN_CL, syms=None, hlit_field=None, hdist_field=None):
    """a dynamic block's header as it is told to: HLIT and HDIST from the lengths unless the fields are given, HCLEN, the
    code-length code's lengths, and the code-length symbols [(symbol, extra or None) or ("raw", code, bits)], by default
    one per length"""
    w.put(final, 1); w.put(2, 2)
    a = w.n
    w.put(len(ll) - 257 if hlit_field is None else hlit_field, 5)
    w.put(len(dd) - 1 if hdist_field is None else hdist_field, 5)
    w.put(hclen - 4, 4)
    w.region("hlit-hdist-hclen", a)
    a = w.n
    assert all(cl[s] == 0 for s in ORDER[hclen:])
    for s in ORDER[:hclen]:
        w.put(cl[s], 3)
    w.region("code-length-lengths", a)
    cc = canonical(cl)
    for t in plain(list(ll) + list(dd)) if syms is None else syms:
        if t[0] == "raw":
            w.code(t[1], t[2])
            continue
        s, extra = t
        w.code(*cc[s])
        if s >= 16:
            a = w.n
            w.put(extra, {16: 2, 17: 3, 18: 7}[s])
            w.region("extra-of-%d" % s, a)
    return Coder(w, ll, dd)


def fib_table():
    """a dynamic table with literal/length codes of up to 15 bits and distance codes beyond 9 (more than the kernels' fast tables
    index: LBITS = 11, DBITS = 9): Fibonacci-like counts make the deepest Huffman trees"""
    ll = (C.c_uint32 * 286)(*([1] * 286))
    dd = (C.c_uint32 * 30)(*([1] * 30))
    a, b = 1, 2
    for k in range(24):
        ll[97 + k] = b
        a, b = b, a + b
    a, b = 1, 2
    for k in range(20):
        dd[29 - k] = b                                  # the SHORT distances keep the long codes
        a, b = b, a + b
    dht, dhtlen = O.dhtgen(ll, dd)
    codes = O.Codes()
    assert O.lib().nxo_dht_parse(dht, dhtlen, C.byref(codes)) == dhtlen
    return dht, dhtlen, codes


def hand_lengths():
    """hand_table()'s code lengths (ll, dd)"""
    ll = [9] * 286
    for sym, n in ((101, 2), (32, 3), (116, 4), (97, 7), (111, 8), (110, 8)):       # Kraft sum 1 with 280 codes of 9 bits
        ll[sym] = n
    L = 9
    for k in range(6):                                     # {L, 9, 9} -> {L + 1, 8, L + 1}: the sum stays, the longest code grows
        ll[206], ll[120 + k], ll[200 + k] = L + 1, 8, L + 1
        L += 1
    chain = [4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 15]
    dd = chain[::-1] + [2, 3, 4] + [5] * 14                # distance symbols 0..6 (distances 1..12): 15, 15, 14, 13, 12, 11, 10 bits
    assert len(ll) == 286 and len(dd) == 30
    return ll, dd


def hand_table(lengths=None):
    """a complete code written by hand in which both alphabets reach 15 bits (O.dhtgen stops at 14 and 12 on any counts): every
    symbol has a code, bytes 200..206 and the distances 1..12 have those of 10 to 15 bits.  Returns (bit string, bits)."""
    ll, dd = lengths or hand_lengths()
    v, n = 0, 0

    def put(val, nbits):
        nonlocal v, n
        v |= val << n
        n += nbits
    put(29, 5); put(29, 5); put(15, 4)                      # HLIT, HDIST, HCLEN = 19
    for sym in (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15):
        put(4 if sym < 16 else 0, 3)                       # the code-length code: sixteen codes of 4 bits, symbol k = code k
    for x in ll + dd:
        put(int(format(x, "04b")[::-1], 2), 4)
    return v.to_bytes((n + 7) // 8, "little"), n


# ---- the cases ------------------------------------------------------------------------------------------------------------

def _noise(n, seed):
    out, x = bytearray(), seed * 2654435761 % (1 << 32) or 1
    for _ in range(n):
        x = (x * 1103515245 + 12345) & 0x7fffffff
        out.append(x >> 16 & 0xff)
    return bytes(out)


HIST = _noise(32768, 5)


def _table_block(w, table, nbits, ll, dd, final=1):
    """a dynamic block whose table is there as a bit string"""
    w.put(final, 1); w.put(2, 2)
    w.bits(table, nbits)
    return Coder(w, ll, dd)


def _long_code_text(c, ll, dd):
    """literals, lengths and distances with the longest codes of each alphabet among them: every byte value, every length
    symbol, every distance symbol (32 KiB of history in front)"""
    c.lits(bytes(range(256)))
    c.lits(bytes(range(200, 207)) * 2)
    for d in range(1, 13):
        c.match(3 + d, d)
    for s in range(29):
        c.length(257 + s, 0); c.dist(s % 7, 0)
    for s in range(30):
        c.length(257, 0); c.dist(s, (1 << DEXTRA[s]) - 1)
    used_l = [ll[b] for b in range(256)], [ll[257 + s] for s in range(29)]
    assert max(used_l[0]) == max(ll[:256]) and max(used_l[1]) == max(ll[257:]) and max(dd) == max(dd[:30])


def _valid():
    out = []

    def add(name, w, hist=b""):
        out.append(("valid/" + name, w, hist))

    w = Bits(); stored(w, b"", 1)
    add("a-final-stored-block-of-length-0", w)
    for n in (0, 1, 65535):
        w = Bits()
        c = fixed(w); c.lits(b"ab"); c.eob()
        stored(w, _noise(n, 9))
        c = fixed(w, 1); c.match(5, min(n + 2, 32768)); c.eob()
        add("a-stored-block-of-length-%d-between-huffman-blocks" % n, w)
    for b in range(8):
        w = Bits()
        c = fixed(w); c.lits(bytes([200] * b)); c.eob()     # 3 + 9 b + 7 bits
        at = w.n % 8
        stored(w, b"stored", 1)
        add("a-stored-block-whose-header-starts-at-bit-%d" % at, w)
    assert sorted(n[0][-1] for n in out[-8:]) == list("01234567")
    w = Bits(); fixed(w, 1).eob()
    add("a-fixed-block-of-end-of-block-only", w)
    w = Bits()
    for k in range(40):
        c = fixed(w); c.lits(bytes([65 + k % 26])); c.eob()
        stored(w, bytes([48 + k % 10]))
    c = fixed(w, 1); c.match(80, 80); c.eob()
    add("forty-one-literal-blocks-and-one-byte-stored-blocks-and-a-match-across-all", w)
    w = Bits(); c = fixed(w, 1); c.lits(b"a"); c.match(258, 1); c.eob()
    add("length-258-as-symbol-285", w)
    w = Bits(); c = fixed(w, 1); c.lits(b"a"); c.match(258, 1, lsym=284); c.eob()
    add("length-258-as-symbol-284-and-31", w)
    for code, mk in (("fixed", lambda w: fixed(w, 1)), ("dynamic", lambda w: dynamic(w, 1, GEN_LL, GEN_DD))):
        for how in ("lowest", "highest"):
            w = Bits(); c = mk(w); c.lits(b"abcdefgh")
            for s in range(29):
                c.length(257 + s, (1 << LEXTRA[s]) - 1 if how == "highest" else 0); c.dist(5, 1)      # distance 8
            c.eob()
            add("%s-code-every-length-symbol-at-its-%s-extra" % (code, how), w)
            w = Bits(); c = mk(w)
            for s in range(30):
                c.length(257, 0); c.dist(s, (1 << DEXTRA[s]) - 1 if how == "highest" else 0)
            c.eob()
            add("%s-code-every-distance-symbol-at-its-%s-extra" % (code, how), w, HIST)
    for s in range(30):                                    # the history is exactly as long as the symbol's farthest distance
        far = DBASE[s] + (1 << DEXTRA[s]) - 1
        w = Bits(); c = fixed(w, 1)
        c.length(257, 0); c.dist(s, (1 << DEXTRA[s]) - 1)
        c.length(257, 0); c.dist(s, 0)
        c.eob()
        add("distance-symbol-%02d-at-both-extras-into-%d-bytes-of-history" % (s, far), w, HIST[-far:])
    w = Bits(); c = fixed(w, 1); c.lits(HIST[:32768].translate(bytes(i % 144 for i in range(256)))); c.match(258, 32768); c.eob()
    add("distance-32768-with-32768-bytes-from-the-stream-in-front", w)
    w = Bits(); c = fixed(w, 1); c.match(258, 32768); c.eob()
    add("distance-32768-with-32768-bytes-of-history-in-front", w, HIST)
    w = Bits(); c = fixed(w, 1); c.lits(b"x"); c.match(258, 1); c.lits(b"y"); c.eob()
    add("distance-1-length-258-the-overlapping-copy", w)
    w = Bits(); c = fixed(w, 1); c.lits(b"abc"); c.match(258, 3); c.eob()
    add("a-match-whose-last-byte-is-the-last-of-the-target", w)
    small = [0] * 258; small[97], small[256], small[257] = 1, 2, 2
    w = Bits(); c = dynamic(w, 1, small, [1]); c.lits(b"a"); c.match(3, 1); c.lits(b"a"); c.eob()
    add("dynamic-one-distance-code-of-length-1", w)
    w = Bits(); c = dynamic(w, 1, small, [0]); c.lits(b"aaa"); c.eob()
    add("dynamic-all-distance-lengths-zero-and-literals-only", w)
    only = [0] * 257; only[256] = 1
    w = Bits(); c = dynamic(w, 1, only, [0]); c.eob()
    add("dynamic-block-of-end-of-block-only", w)
    eights = [8] * 255 + [0, 8]
    cl5 = [0] * 19; cl5[0], cl5[8] = 1, 1
    w = Bits(); c = dynamic(w, 1, eights, [0], hclen=5, cl=cl5); c.lits(bytes(range(255))); c.eob()
    add("hclen-5-the-lowest-that-can-code-an-end-of-block", w)
    w = Bits(); c = dynamic(w, 1, GEN_LL, GEN_DD); c.lits(b"hclen nineteen"); c.match(9, 8); c.eob()
    add("hclen-19", w)
    # code-length repeats: 138 symbols of no code in front of 108 codes of 7 bits and 40 of 8
    runs_ll = [0] * 138 + [7] * 108 + [8] * 40
    assert kraft(runs_ll) == 1.0
    for s, k, rest in ((16, 3, []), (16, 6, []), (17, 3, [(3, 18, 135)]), (17, 10, [(10, 18, 128)]), (18, 11, [(11, 18, 127)]), (18, 138, [])):
        runs = [(139, 16, k)] if s == 16 else [(0, s, k)] + rest
        w = Bits(); c = dynamic(w, 1, runs_ll, GEN_DD, syms=with_runs(runs_ll + GEN_DD, runs))
        c.lits(bytes(range(138, 256))); c.match(20, 100); c.eob()
        add("code-length-repeat-%d-of-%d-entries" % (s, k), w)
    # runs that begin in the literal/length lengths and end in the distance lengths
    ll16, dd16 = [9] * 102 + [8] * 181 + [5] * 3, [5, 5, 5, 4, 4] + [5] * 25
    assert kraft(ll16) == kraft(dd16) == 1.0
    w = Bits(); c = dynamic(w, 1, ll16, dd16, syms=with_runs(ll16 + dd16, [(284, 16, 5)]))
    c.lits(b"crossing"); c.match(258, 8, lsym=284); c.length(285, 0); c.dist(0, 0); c.eob()
    add("a-run-of-16-from-the-literal-lengths-into-the-distance-lengths", w)
    for s, hlit, k in ((17, 260, 6), (18, 270, 16)):
        llx = [8] * 254 + [0, 0, 7] + [0] * (hlit - 257)
        ddx = [0, 0, 0, 1]
        assert kraft(llx) == 1.0
        w = Bits(); c = dynamic(w, 1, llx, ddx, syms=with_runs(llx + ddx, [(257, s, k)]))
        c.lits(b"crossing"); c.eob()
        add("a-run-of-%d-from-the-literal-lengths-into-the-distance-lengths" % s, w)
    w = Bits(); c = dynamic(w, 1, eights, [1, 1]); c.lits(b"hlit 257"); c.eob()
    add("hlit-257", w)
    w = Bits(); c = dynamic(w, 1, GEN_LL, [1, 1]); c.lits(b"hlit 286"); c.length(285, 0); c.dist(1, 0); c.eob()
    add("hlit-286", w)
    ll260 = [8] * 253 + [0, 0, 0, 8, 8, 0, 8]                 # 256 codes of 8 bits, HLIT 260
    assert kraft(ll260) == 1.0
    w = Bits(); c = dynamic(w, 1, ll260, [1]); c.lits(b"hdist 1"); c.match(3, 1); c.eob()
    add("hdist-1", w)
    w = Bits(); c = dynamic(w, 1, ll260, GEN_DD); c.lits(b"hdist 30"); c.length(257, 0); c.dist(29, 7); c.eob()
    add("hdist-30", w, HIST)
    # codes of 15 bits
    hl, hd = hand_lengths()
    t, nb = hand_table()
    w = Bits(); c = _table_block(w, t, nb, hl, hd); _long_code_text(c, hl, hd); c.eob()
    assert max(hl) == 15 and max(hd) == 15
    add("the-15-15-bit-table-written-by-hand-with-its-longest-codes-in-use", w, HIST)
    t, nb, codes = fib_table()
    fl, fd = list(codes.ll_len)[:286], list(codes.d_len)[:30]
    w = Bits(); c = _table_block(w, t, nb, fl, fd); _long_code_text(c, fl, fd); c.eob()
    add("the-fibonacci-table-with-its-longest-codes-in-use", w, HIST)
    el = list(hl); el[256], el[205] = hl[205], hl[256]
    assert el[256] == 15 and kraft(el) == 1.0
    t, nb = hand_table((el, hd))
    w = Bits(); c = _table_block(w, t, nb, el, hd); _long_code_text(c, el, hd); c.eob()
    add("the-15-bit-table-with-a-15-bit-end-of-block", w, HIST)
    for text in [b"e" * k + tail for k in range(4) for tail in (b"", b" ")]:       # ('e' has 2 bits in that table, ' ' 3)
        w = Bits(); c = _table_block(w, t, nb, el, hd); c.lits(text); c.eob()
        if w.n % 8 == 0:
            break
    assert w.n % 8 == 0
    add("a-block-whose-longest-code-ends-in-the-last-bit-of-the-source", w)
    return out


def _lenient():
    out = []
    inc = [0] * 258; inc[97], inc[256], inc[257] = 2, 2, 2                          # three codes of 2 bits: 11 has no symbol
    w = Bits(); c = dynamic(w, 1, inc, [1]); c.lits(b"a"); c.match(3, 1); c.eob()
    out.append(("lenient/an-incomplete-literal-length-code-of-which-only-assigned-codes-are-used", w, b""))
    small = [0] * 258; small[97], small[256], small[257] = 1, 2, 2
    w = Bits(); c = dynamic(w, 1, small, [2, 2]); c.lits(b"aa"); c.match(3, 1); c.match(3, 2); c.eob()
    out.append(("lenient/an-incomplete-distance-code-of-which-only-assigned-codes-are-used", w, b""))
    cl = list(GEN_CL); cl[15] = 0                                                  # (the last code of 5 bits: the others stay)
    w = Bits(); c = dynamic(w, 1, small, [1], cl=cl); c.lits(b"a"); c.match(3, 1); c.eob()
    out.append(("lenient/an-incomplete-code-length-code-of-which-only-assigned-codes-are-used", w, b""))
    return out


def _errors():
    """[(name, f(w, bytes in front: output and history), history)]: f writes the block that is wrong and nothing behind what is wrong"""
    small = [0] * 258; small[97], small[256], small[257] = 1, 2, 2
    inc = [0] * 258; inc[97], inc[256], inc[257] = 2, 2, 2
    E = []

    def err(name, hist=b""):
        def deco(f):
            E.append((name, f, hist))
            return f
        return deco

    @err("a-stored-block-whose-nlen-is-not-the-complement-of-len")
    def _(w, front):
        stored(w, b"", 1, nlen=0xfff0)

    @err("btype-3")
    def _(w, front):
        w.put(1, 1); w.put(3, 2)

    @err("fixed-code-length-symbol-286")
    def _(w, front):
        c = fixed(w, 1); c.lits(b"a"); c.sym(286)

    @err("fixed-code-length-symbol-287")
    def _(w, front):
        c = fixed(w, 1); c.lits(b"a"); c.sym(287)

    @err("fixed-code-distance-symbol-30")
    def _(w, front):
        c = fixed(w, 1); c.lits(b"a"); c.length(257, 0); c.dist(30, 0)

    @err("fixed-code-distance-symbol-31")
    def _(w, front):
        c = fixed(w, 1); c.lits(b"a"); c.length(257, 0); c.dist(31, 0)

    @err("a-distance-one-beyond-the-output")
    def _(w, front):
        c = fixed(w, 1); c.lits(b"a"); c.match(3, front + 2)

    @err("a-distance-one-beyond-the-output-and-the-history", HIST[:100])
    def _(w, front):
        c = fixed(w, 1); c.lits(b"a"); c.match(3, front + 2)

    @err("an-over-subscribed-literal-length-code")
    def _(w, front):
        ll = list(small); ll[98] = 1
        dynamic(w, 1, ll, [1])

    @err("an-over-subscribed-distance-code")
    def _(w, front):
        dynamic(w, 1, small, [1, 1, 1])

    @err("an-over-subscribed-code-length-code")
    def _(w, front):
        cl = list(GEN_CL); cl[18] = 4
        w.put(1, 1); w.put(2, 2); w.put(1, 5); w.put(0, 5); w.put(15, 4)
        for s in ORDER:
            w.put(cl[s], 3)

    @err("a-table-with-no-end-of-block-code")
    def _(w, front):
        ll = [0] * 258; ll[97], ll[98] = 1, 1
        dynamic(w, 1, ll, [1])

    @err("a-repeat-as-the-first-code-length-symbol")
    def _(w, front):
        dynamic(w, 1, small, [1], syms=[(16, 0)])

    @err("a-repeat-run-past-hlit-and-hdist")
    def _(w, front):
        llx = [8] * 254 + [0, 0, 7, 0, 0, 0]
        dynamic(w, 1, llx, [0, 0, 0, 1], syms=plain(llx[:257]) + [(18, 127)])

    for field in (30, 31):
        @err("hlit-field-%d-%d-literal-length-codes" % (field, 257 + field))
        def _(w, front, field=field):
            w.put(1, 1); w.put(2, 2); w.put(field, 5); w.put(0, 5); w.put(15, 4)

        @err("hdist-field-%d-%d-distance-codes" % (field, 1 + field))
        def _(w, front, field=field):
            w.put(1, 1); w.put(2, 2); w.put(0, 5); w.put(field, 5); w.put(15, 4)

    @err("use-of-an-unassigned-literal-length-code")
    def _(w, front):
        c = dynamic(w, 1, inc, [1]); c.lits(b"a"); c.raw(3, 2)

    @err("use-of-an-unassigned-distance-code")
    def _(w, front):
        c = dynamic(w, 1, small, [2]); c.lits(b"a"); c.length(257, 0); c.raw(1, 2)

    @err("use-of-an-unassigned-code-length-code")
    def _(w, front):
        cl = list(GEN_CL); cl[15] = 0
        dynamic(w, 1, small, [1], cl=cl, syms=plain(small[:100]) + [("raw", 31, 5)])

    @err("a-match-in-a-block-with-no-distance-code")
    def _(w, front):
        c = dynamic(w, 1, small, [0]); c.lits(b"a"); c.length(257, 0); w.put(0, 1)

    @err("hclen-4-which-cannot-code-an-end-of-block")
    def _(w, front):
        cl = [0] * 19; cl[0], cl[18] = 1, 1
        ll = [0] * 257
        dynamic(w, 1, ll, [0], hclen=4, cl=cl, syms=[(18, 127), (18, 98), (18, 0)])

    return E


GOOD = 30 * 1024                                           # output in front of a third block


def _good_blocks(w):
    """two blocks of 30 KiB of output: a stored one and a fixed one"""
    stored(w, _noise(15000, 3))
    c = fixed(w)
    c.lits(b"thirty kibibytes of good output ")
    n = 15000 + 32
    while n + 258 <= GOOD:
        c.match(258, 32 if n % 3 else 15032); n += 258
    c.lits(b"z" * (GOOD - n))
    c.eob()


def _error_cases():
    out = []
    for name, f, hist in _errors():
        w = Bits(); f(w, len(hist))
        out.append(("error/%s/at-the-end" % name, w.data(), hist))
        out.append(("error/%s/padded" % name, w.data() + bytes(8), hist))
        w = Bits(); _good_blocks(w); f(w, GOOD + len(hist))
        out.append(("error/%s/third-block" % name, w.data() + bytes(8), hist))
    return out


def _target():
    out = []
    w = Bits(); c = fixed(w, 1); c.lits(b"a")
    for _ in range(CAP_REST // 258 + 1):
        c.match(258, 1)
    c.eob()
    out.append(("target/a-match-runs-over-the-capacity", w.data(), b""))
    w = Bits(); c = fixed(w, 1); c.lits(b"ab")
    for _ in range((CAP_REST - 2) // 258):
        c.match(258, 2)
    c.lits(b"c" * (CAP_REST - 2 - (CAP_REST - 2) // 258 * 258 + 1)); c.eob()
    out.append(("target/a-literal-runs-over-the-capacity", w.data(), b""))
    w = Bits(); stored(w, _noise(CAP_REST - 10, 4)); stored(w, _noise(11, 6), 1)
    out.append(("target/a-stored-block-runs-over-the-capacity", w.data(), b""))
    return out


def _cuts(valid):
    """of every kind of place, up to six valid streams cut at a byte inside it (spread over those that have such a byte).
    Not every valid stream at every place: where a decoder stops when the source ends is decided by the field it ends in
    -- each kernel has one path a field -- not by what the stream holds elsewhere, so a kind is pinned by a few streams that
    put the field at different bits of a byte and behind different amounts of output; six a kind keep the batch small (42
    of the 187 cases).  The pick is by position in _valid()'s list, so a case added there may move it: the case names say
    which stream and which byte, and the host test asks of every kind that it is there and stops where it says."""
    out = []
    for kind in CUT_KINDS:
        found = []
        for name, w, hist in valid:
            if w.n > 8 * CAP_REST:                         # (the stored block of 65535 bytes: its output does not fit CAP_REST)
                continue
            for k, a, b in w.regions:
                cut = (b - 1) // 8                         # the last byte boundary in front of the region's last bit
                if k == kind and (a < 8 * cut or (a == 8 * cut and kind in CUT_KINDS[2:6])):
                    found.append(("cut/%s/byte-%d-of-%s" % (kind, cut, name[6:]), w.data()[:cut], hist))
                    break
        step = max(1, len(found) // 6)
        out += found[::step][:6]
    return out


_cases = None
_records = None


def cases():
    """[(name, stream, history)] (built once a process)"""
    global _cases
    if _cases is None:
        valid = _valid()
        done = [(n, w.data(), h) for n, w, h in valid + _lenient()]
        _cases = done + _error_cases() + _target() + _cuts(valid)
        assert len(set(n for n, _, _ in _cases)) == len(_cases)
    return _cases


def family(name):
    return name.split("/")[0]


def records():
    """the cases with the oracle's answer to each: Rec (built once a process; fields named as tests/resume_cases.py's Case)"""
    global _records
    if _records is None:
        _records = []
        for name, src, hist in cases():
            fam = family(name)
            cap = CAP_REST
            if fam in ("valid", "lenient"):
                cap = O.inflate(src, 1 << 17, hist=hist)[1].tpbc
            out, st = O.inflate(src, cap, hist=hist)
            _records.append(Rec(name, fam, src, hist, cap, out, st.err, st.tpbc, bool(st.final_eob), st.out_sfbt, st.out_subc,
                                st.out_rembytecnt, bytes(st.out_dht), st.out_dhtlen, 0, 1))
    return _records


def zlib_verdict(src, hist, cap):
    """("end", bytes) when zlib reaches the end of the stream within cap bytes, ("error", message), or ("more", bytes)"""
    d = zlib.decompressobj(-15, zdict=hist) if hist else zlib.decompressobj(-15)
    try:
        out = d.decompress(src, cap + 1)
    except zlib.error as e:
        return "error", str(e)
    return ("end" if d.eof and len(out) <= cap else "more"), out
