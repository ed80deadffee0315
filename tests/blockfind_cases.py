"""Streams for the block search (power-gzip_amd/csrc/nxz_blockfind.hip), written with tests/deflate_handmade.py's bit writer:
dynamic block HEADERS -- the search reads nothing else -- at chosen bit positions of seeded random bytes.  What passes, in
the headers and in the random bytes between them alike, is for tests/blockfind_model.py to say: nothing here is assumed to
be noise that cannot pass.

HEADERS: name -> (bytes, bits, the model's verdict when it stands alone: "ok" or the reason it fails for).  Those that fail
are one edit away from one that passes.
cases(S): [Case] for segments of S bytes (512 and 1024: all of them; 2048 and 8192: a subset -- those that are about the edges
of a segment, of the stream and of the kernel's passes over 8192 positions, the overflow, two of the headers, and a stream off a
16-byte boundary and a first_bit inside the second pass; the model costs seconds per 100 KiB of stream).
Case.offset: where the stream lies relative to a 16-byte boundary of memory (the two branches of load_segment).

RFC 1951 leaves no header with HCLEN 4 that can pass (the four lengths sent are those of 16, 17, 18 and 0: no length but
zero can be coded, so end-of-block has no code): the smallest header here has HCLEN 5, HLIT 257, HDIST 1, and HCLEN 4 is
among those that must not pass, for "no-256" and not for its last length, which is zero and exempt from the trimming rule."""
import random
from collections import namedtuple

import deflate_handmade as H

Case = namedtuple("Case", "name src first_bit offset seg placed")

SMALL = [0] * 258
SMALL[97], SMALL[256], SMALL[257] = 1, 2, 2
EIGHTS = [8] * 255 + [0, 8]                                # 256 codes of 8 bits, HLIT 257
CL5 = [0] * 19
CL5[0], CL5[8] = 1, 1                                      # HCLEN 5
CL_SHORT = [0] * 19
CL_SHORT[18], CL_SHORT[0], CL_SHORT[1], CL_SHORT[2] = 1, 2, 3, 3
SHORT_RUNS = [(0, 18, 97), (98, 18, 138), (236, 18, 20)]
CL_SEVEN = [0] * 19                                        # four codes of 7 bits (4, 5, 8, 9), and 1..5 bits
for _s, _l in ((0, 1), (16, 2), (17, 3), (18, 4), (1, 5), (4, 7), (5, 7), (8, 7), (9, 7)):
    CL_SEVEN[_s] = _l
CL_REP7 = [0] * 19                                         # the repeats 16 and 18 have the codes of 7 bits
for _s, _l in ((0, 1), (8, 2), (7, 3), (9, 4), (6, 5), (17, 6), (16, 7), (18, 7)):
    CL_REP7[_s] = _l
RUNS_LL = [0] * 138 + [7] * 108 + [8] * 40
LL16, DD16 = [9] * 102 + [8] * 181 + [5] * 3, [5, 5, 5, 4, 4] + [5] * 25
INC = [0] * 258
INC[97], INC[256], INC[257] = 2, 2, 2
CL_SIG = [0] * 19
CL_SIG[0], CL_SIG[8], CL_SIG[1] = 1, 2, 2                  # (symbol 15, the last that is sent, has no code)
assert all(H.kraft(c) == 1.0 for c in (CL5, CL_SHORT, CL_SEVEN, CL_REP7, CL_SIG, RUNS_LL, LL16, DD16, EIGHTS))


def _hclen(cl):
    return max(4, max(i + 1 for i, s in enumerate(H.ORDER) if cl[s]))


def _hdr(ll, dd, cl=H.GEN_CL, hclen=None, final=0, **kw):
    w = H.Bits()
    H.dynamic(w, final, ll, dd, hclen=hclen or _hclen(cl), cl=cl, **kw)
    return w.data(), w.n


def _headers():
    out = {}

    def add(name, verdict, *a, **kw):
        out[name] = _hdr(*a, **kw) + (verdict,)

    # ---- must pass
    add("the-smallest-hclen-5-hlit-257-hdist-1", "ok", EIGHTS, [0], cl=CL5)
    add("short", "ok", SMALL, [1], cl=CL_SHORT, syms=H.with_runs(SMALL + [1], SHORT_RUNS))
    add("short-final", "ok", SMALL, [1], cl=CL_SHORT, syms=H.with_runs(SMALL + [1], SHORT_RUNS), final=1)
    add("a-distance-code-that-is-empty", "ok", SMALL, [0])
    add("a-distance-code-that-is-a-single-1-bit-code", "ok", SMALL, [1])
    add("a-single-1-bit-distance-code-behind-three-without", "ok", SMALL, [0, 0, 0, 1])
    add("a-complete-distance-code", "ok", H.GEN_LL, H.GEN_DD)      # (286 / 30 / 19 with nothing trimmed)
    ll285 = [9] * 58 + [8] * 227
    assert H.kraft(ll285) == 1.0
    add("a-complete-distance-code-hlit-285", "ok", ll285, H.GEN_DD)
    add("the-286-30-19-signature-with-trailing-zero-lengths", "ok", EIGHTS + [0] * 29, [1] + [0] * 29, cl=CL_SIG, hclen=19)
    add("a-16-run-across-hlit-into-the-distance-lengths", "ok", LL16, DD16, syms=H.with_runs(LL16 + DD16, [(284, 16, 5)]))
    add("an-18-run-of-138", "ok", RUNS_LL, H.GEN_DD, syms=H.with_runs(RUNS_LL + H.GEN_DD, [(0, 18, 138)]))
    add("the-longest-every-length-a-7-bit-code", "ok", H.GEN_LL, H.GEN_DD, cl=CL_SEVEN, hclen=19)
    add("7-bit-codes-for-the-repeats", "ok", RUNS_LL, [0], cl=CL_REP7, syms=H.with_runs(RUNS_LL + [0], [(0, 18, 138), (139, 16, 6)]))
    add("7-bit-code-for-18-only-in-use", "ok", RUNS_LL, [0], cl=CL_REP7, syms=H.with_runs(RUNS_LL + [0], [(0, 18, 138)]))
    add("a-16-run-that-ends-at-the-total", "ok", LL16, DD16, syms=H.with_runs(LL16 + DD16, [(311, 16, 5)]))
    # ---- must not
    add("trailing-zero-literal-lengths-without-the-signature", "trim-hlit", EIGHTS + [0] * 28, [1])
    add("trailing-zero-distance-lengths-without-the-signature", "trim-hdist", SMALL, [1, 0, 0, 0])
    add("hlit-30", "hlit", EIGHTS, [0], cl=CL5, hlit_field=30)
    add("hdist-30", "hdist", EIGHTS, [0], cl=CL5, hdist_field=30)
    over = list(CL_REP7); over[5] = 7
    add("code-length-code-one-unit-over", "cl-over", RUNS_LL, [0], cl=over, syms=H.with_runs(RUNS_LL + [0], [(0, 18, 138)]))
    under = list(CL_REP7); under[16] = 0
    add("code-length-code-one-unit-under", "cl-under", RUNS_LL, [0], cl=under, hclen=_hclen(CL_REP7), syms=H.with_runs(RUNS_LL + [0], [(0, 18, 138)]))
    add("no-code-for-256", "no-256", [8] * 256 + [0], [0], cl=CL5)
    add("an-incomplete-literal-length-code", "ll-under", INC, [1])
    o = list(SMALL); o[98] = 1
    add("an-oversubscribed-literal-length-code", "ll-over", o, [1])
    add("a-distance-code-of-two-codes-of-length-2", "dist-under", SMALL, [2, 2])
    add("a-16-as-the-first-symbol", "repeat-first", SMALL, [1], syms=[(16, 0)] + H.plain(SMALL[3:] + [1]))
    syms = H.with_runs(LL16 + DD16, [(311, 16, 5)])
    assert syms[-1] == (16, 2)
    add("a-run-that-overshoots-the-total-by-1", "overrun", LL16, DD16, syms=syms[:-1] + [(16, 3)])
    add("the-last-hclen-length-zero-with-hclen-6", "trim-hclen", EIGHTS, [0], cl=CL5, hclen=6)
    cl4 = [0] * 19; cl4[17], cl4[18] = 1, 1
    add("hclen-4-which-cannot-code-an-end-of-block", "no-256", [0] * 257, [0], cl=cl4, hclen=4, syms=[(18, 127), (18, 98), (18, 0)])
    return out


HEADERS = _headers()
MUST_PASS = [k for k, v in HEADERS.items() if v[2] == "ok"]
MUST_NOT = [k for k, v in HEADERS.items() if v[2] != "ok"]
LONGEST = "the-longest-every-length-a-7-bit-code"
assert HEADERS[LONGEST][1] == 17 + 19 * 3 + 316 * 7
POISON = 0xa5


def filler(n, seed):
    return bytearray(random.Random(seed).randbytes(n))


def place(buf, bit, name):
    """the header's bits over those of buf from `bit` on (what of it lies behind buf's end is lost: a cut header)"""
    data, n, _ = HEADERS[name]
    for k in range(n):
        at = bit + k
        if at >= 8 * len(buf):
            break
        b = data[k >> 3] >> (k & 7) & 1
        buf[at >> 3] = (buf[at >> 3] & ~(1 << (at & 7))) | b << (at & 7)


def _case(name, S, n, seed, placed, first_bit=0, offset=0):
    buf = filler(n, seed)
    for bit, h in placed:
        place(buf, bit, h)
    return Case("%s/seg-%d" % (name, S), bytes(buf), first_bit, offset, S, tuple(placed))


def overflow_stream(S):
    """a short header that passes every 107 bits (its length): 76 to a KiB -- more than the 126 the first kernel hands to the second
    in every segment of 2 KiB or more"""
    n = (3 if S <= 1024 else 2) * S + 200
    return [(p, "short") for p in range(5, 8 * n - 120, 107)], n


def cases(S):
    full = S <= 1024
    sb = 8 * S
    out = []
    nshort = HEADERS["short"][1]

    def add(name, n, placed, **kw):
        out.append(_case(name, S, n, len(out) + 7 * S, placed, **kw))

    # ---- placement at the edges of a segment (the long segments: in streams of two and a bit)
    e = 2 * sb if full else sb
    ne = e // 8 + S + 77
    add("at-the-first-bit-of-a-segment", ne, [(e, "short")])
    add("the-longest-header-at-the-last-bit-of-a-segment", ne + S, [(e - 1, LONGEST), (e + sb - 1, "short")])
    add("16-bits-in-front-of-the-end-of-a-segment", ne + S, [(e - 16, "short"), (e + sb - 13, "short")] + ([(sb - 12, "short")] if full else []))
    if full:
        add("either-side-of-a-32-bit-boundary", 4 * S + 77, [(31, "short"), (sb + 32, "short"), (2 * sb + 33, "short"), (3 * sb + 63, "short")])
    if S >= 2048:
        add("either-side-of-a-pass-of-8192-positions", 2 * S + 77, [(8191, "short"), (8192 + 107, "short"), (sb + 8193, "short"), (sb + 8192 - 130, "short")])
    # ---- placement at the end of the stream
    n = (3 if full else 1) * S + 300
    add("ending-at-the-last-bit-of-the-stream", n, [(8 * n - nshort, "short")])
    add("ending-at-the-last-bit-of-the-stream-the-longest", n, [(8 * n - HEADERS[LONGEST][1], LONGEST)])
    add("cut-by-1-bit-by-the-end-of-the-stream", n, [(8 * n - nshort + 1, "short")])
    add("cut-by-17-bits-by-the-end-of-the-stream", n, [(8 * n - nshort + 17, "short")])
    add("cut-in-the-code-length-lengths-by-the-end-of-the-stream", n, [(8 * n - 17 - 20, "short")])
    add("cut-in-the-first-17-bits-by-the-end-of-the-stream", n, [(8 * n - 10, "short"), (8 * n - 16, "short-final")])
    g = 4 if full else 1
    add("in-a-last-segment-shorter-than-16-bytes", g * S + 15, [(g * sb + 3, "short")])
    add("in-a-last-segment-whose-length-is-no-multiple-of-16", g * S + 53, [(g * sb + 38 * 8 + 2, "short")])
    # ---- how many in a segment: `more` with and without spare entries
    if full:
      add("two-three-four-and-five-in-a-segment-and-none", 5 * S + 100,
          [(g * sb + 11 + k * (nshort + 3 + 64 * g), "short" if k % 2 else "short-final") for g in range(4) for k in range(g + 2)])
    placed, n = overflow_stream(S)
    add("a-short-header-every-107-bits", n, placed)
    # ---- every header
    names = MUST_PASS + MUST_NOT
    for i in range(0, len(names), 4):
        add("headers-%02d" % (i // 4), (4 if full else 2) * S + 200 + i, [(g * sb + 8 * 37 + (3 * i + g) % 8, h) for g, h in enumerate(names[i:i + (4 if full else 2)])])
        if not full:
            break
    if not full:
        # (segments of more than one pass of 8192 positions: the byte branch of load_segment, and a first_bit inside the second pass)
        placed = [(8192 - 40, "short"), (8192 + 300, "short-final"), (8192 + 900, "short"), (sb - 1, LONGEST), (sb + 8192 + 77, "short")]
        for off in (3, 13):
            out.append(_case("the-stream-at-offset-%d-from-a-16-byte-boundary" % off, S, 2 * S + 53, 993, placed, offset=off))
        for fb in (8192 + 300, 8192 + 301, 8192 + 320, sb + 8192 + 64):
            out.append(_case("first-bit-in-the-second-pass-%d" % fb, S, 2 * S + 53, 993, placed, first_bit=fb))
        assert len(set(c.name for c in out)) == len(out)
        return out
    # ---- all 8 bit offsets of a byte
    for half in (0, 1):
        add("at-bit-offsets-%d-to-%d-of-a-byte" % (4 * half, 4 * half + 3), 4 * S + 60, [(g * sb + 808 + 4 * half + g, "short") for g in range(4)])
    # ---- first_bit
    placed = [(40, "short"), (300, "short-final"), (sb + 200, "short"), (sb + 900, "short"), (2 * sb + 100, "short")]
    for fb in (0, 1, 7, 31, 32, 33, 39, 40, 41, 63, 64, 65, sb + 500, 2 * sb + 100, 2 * sb + 101):
        out.append(_case("first-bit-%s%d" % ("" if fb < sb else "in-a-later-segment-", fb), S, 3 * S + 60, 991, placed, first_bit=fb))
    # ---- where the stream lies in memory
    for off in (1, 3, 8, 13):
        out.append(_case("the-stream-at-offset-%d-from-a-16-byte-boundary" % off, S, 4 * S + 53, 992,
                         [(2 * sb - 1, LONGEST), (37, "short"), (4 * sb + 38 * 8 + 2, "short")], offset=off))
    assert len(set(c.name for c in out)) == len(out)
    return out


SEGS = (512, 1024, 2048, 8192)
_built = {}


def built(S):
    if S not in _built:
        _built[S] = cases(S)
    return _built[S]


_scans = {}


def scan(c):
    import blockfind_model as M
    if c.src not in _scans:
        _scans[c.src] = M.Scan(c.src)
    return _scans[c.src]


def expected(c, S=None):
    import blockfind_model as M
    return M.expected(c.src, c.first_bit, S or c.seg, scan(c))


def check(c, S, got, two=True):
    """got: `first` as nxz_launch_find_blocks leaves it for case c at segments of S bytes (nseg firsts, then three more a segment);
    two: the two-kernel form.  -> a list of what is wrong (empty: nothing).  Equality as tests/blockfind_model.py segment_class
    defines it: `first` always; `more` when the second kernel certainly did the segment; all ~0 when the first did it itself, or
    alone"""
    import blockfind_model as M
    e = expected(c, S)
    got = [int(x) for x in got]
    assert len(got) == e.nseg * (1 + M.MORE), (c.name, len(got), e.nseg)
    bad = []
    for g in range(e.nseg):
        cls = M.segment_class(e.K[g], e.npass[g])
        assert cls, (c.name, S, g, e.K[g], e.npass[g])
        if got[g] != e.first[g]:
            bad.append("%s: segment %d of %d bytes: first %d, the model %d" % (c.name, g, S, got[g], e.first[g]))
        more = got[e.nseg + g * M.MORE:e.nseg + (g + 1) * M.MORE]
        want = e.more[g] if two and cls == "two" else [M.NONE] * M.MORE
        if more != want:
            bad.append("%s: segment %d of %d bytes: more %s, the model %s" % (c.name, g, S, more, want))
    return bad
