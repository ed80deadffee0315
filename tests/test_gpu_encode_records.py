"""The entropy kernel codes a match record once, when the round's records are copied to LDS (nxz_encode.hip: code_record,
stage_recs), and the lanes only load the finished code.  These blocks sit on the places where that staging can go wrong:
the record count of a 2048-position round at the edges of the staging passes of 256 records, two matches in the four
positions of one quad, the longest and shortest lengths and distances, ragged sizes, a history, and tables that lack a
symbol.  Every block goes through all three forms of the kernel -- the fixed code (encode_kernel<false>: the function codes
with symbol counts, the ones without let the LZ77 kernel write the block), a caller's table (the checked form), the
device's own table (the default form, and the checked form again under NXZ_ENCODE_CHECK=1) -- and is compared with the
CPU oracle byte for byte and inflated with zlib.

What the data reaches is asserted from the oracle's tokens, not assumed.  Two things it does not reach, with this parser:
  * more than 512 records in a round.  A candidate needs four equal bytes (oracle/nxz_lz77.c step 4); a 3-byte match is
    only ever what is left of a longer one at the end of a tile or at the exit X[s] of a 16-position segment (step 5),
    at most one per entered segment, and a segment entered at its own start has none: that bounds a round at
    2048 / 4 = 512 matches on all the word and small-alphabet data tried (493 on random data over 5..24 symbols, 512 on
    dictionary words laid end to end).  The third staging pass (records 512..) is the same unrolled code as the first two.
  * two matches in the LAST quad of a round (the second one starting on the round's last position): a 3-byte match at
    a position 4 mod 8 with a match right behind it is one in 65536 positions of the densest data (five in 1200 seeded
    blocks, none of them at 2044 mod 2048).  The first quad of a lane has them by the dozen, the second is covered once.
"""
import importlib
import os
import zlib

import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu
pkg = importlib.import_module("power-gzip_amd")

STRIDE_IN = 65536
STRIDE_OUT = 73856
RPOS = 2048                       # positions of one round of the kernel
MISSING_CODE = 66                 # NXZ_CC_MISSING_CODE (include/nxz_engine.h)


# ---------------------------------------------------------------------------
# data
# ---------------------------------------------------------------------------
class Lcg:
    def __init__(self, seed):
        self.x = (seed * 2654435761 + 12345) & 0xffffffff

    def next(self, k):
        self.x = (self.x * 1664525 + 1013904223) & 0xffffffff
        return (self.x >> 16) % k


def small_alphabet(seed, n, k):
    """n bytes over k symbols: a match at almost every position, 3-byte ones among them"""
    g = Lcg(seed)
    return bytes(g.next(k) for _ in range(n))


def word_rounds(words_per_round, seed):
    """Round 0 holds 128 four-byte words (first bytes all different); every later round starts with the given number of
    them laid end to end -- no ordered pair of words twice, so every match is exactly one word -- and goes on with bytes
    whose 4-grams never come back."""
    g = Lcg(seed)
    nw = 128
    words = [bytes([i, g.next(256), g.next(256), g.next(256)]) for i in range(nw)]
    used = [[j == i + 1 for j in range(nw)] for i in range(nw)]
    out = bytearray(b"".join(words))
    ctr = [0]

    def fresh(n):
        b = bytearray()
        while len(b) < n:
            c = ctr[0]
            ctr[0] += 1
            b += bytes([(c >> 16) & 0xff, (c >> 8) & 0xff, c & 0xff, (c * 167 + 13) & 0xff])
        return bytes(b[:n])
    out += fresh(RPOS - len(out))
    cur = nw - 1
    for w in words_per_round:
        start = len(out)
        for _ in range(w):
            free = [j for j in range(nw) if not used[cur][j]]
            j = free[g.next(len(free))]
            used[cur][j] = True
            cur = j
            out += words[j]
        out += fresh(RPOS - (len(out) - start))
    assert len(out) <= 65536
    return bytes(out)


def edge_block():
    """strings between runs of zeros (a run takes no part in the match table, so a string is still found 32768 bytes on):
    every (length, distance) below is one string and its copy; periods of 1..5 bytes give the smallest distances"""
    g = Lcg(77)
    buf = bytearray(65536)
    want = []
    pos = 64

    def rnd(n):
        return bytes(1 + g.next(250) for _ in range(n))
    for period in (1, 2, 3, 4, 5):
        unit = rnd(period)
        run = (unit * 400)[:300 + period]              # longer than 258: a match of the full length, and its rest
        buf[pos:pos + len(run)] = run
        pos += len(run) + 40
    # groups of strings and their copies one distance on; no group's strings or copies lie on another's
    edges = [10, 11, 18, 19, 34, 35, 66, 67, 130, 131, 257, 258]
    groups = [(2560, 4096, [4, 5, 6, 7, 8, 9, 12, 13] + edges[:6]),
              (3300, 4097, [14, 15, 16, 17, 22, 23, 26, 27, 30, 31]),
              (8192, 32768, edges + [42, 43, 50, 51, 98, 99] + edges + [162, 163, 226, 227] + edges),
              (22000, 24577, [58, 59, 82, 83, 114, 115, 194, 195])]
    for base, d, lens in groups:
        a = base
        for i, ln in enumerate(lens):
            s = rnd(ln)
            buf[a - 1], buf[a + d - 1] = 253, 254         # another byte in front and behind: the match is the string
            buf[a:a + ln] = s
            buf[a + ln] = 251
            buf[a + d:a + d + ln] = s
            buf[a + d + ln] = 252
            want.append((ln, d))
            a += ln + 21 + i % 7                          # (the copies at changing places in the parser's 16-position segments)
        assert a - base < d and a + d < 65536
    return bytes(buf), want


def match_tokens(data, hist=0):
    """(position, length, distance) of the oracle's match tokens"""
    tok, nt = O.lz77(data, hist)
    out, pos = [], 0
    for i in range(nt):
        t = tok[i]
        if t & O.TOK_MATCH:
            out.append((pos, (t & 0xff) + 3, ((t >> 8) & 0x7fff) + 1))
            pos += (t & 0xff) + 3
        else:
            pos += 1
    assert pos == len(data) - hist
    return out


def round_counts(data):
    c = [0] * ((len(data) + RPOS - 1) // RPOS)
    for p, _, _ in match_tokens(data):
        c[p // RPOS] += 1
    return c


# words per round found with the oracle on the CPU: rounds 1..20 full, then 257, 256, 255 and 1 records with empty rounds between
WORDS = [512] * 20 + [257, 0, 261, 0, 263, 0, 2, 0, 0, 0, 0]
WORDS_SEED = 1
ROUND_COUNTS_WANTED = (0, 1, 255, 256, 257, 512)


# ---------------------------------------------------------------------------
# the three forms
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def eng():
    e = pkg.Engine(0)
    yield e
    e.close()


def universal_table(blocks, hists):
    """a table with a code for every symbol (counts of the first block, none left at zero)"""
    tok, nt = O.lz77(blocks[0], hists[0])
    ll, d = O.counts(tok, nt)
    for i in range(286):
        ll[i] = max(ll[i], 1)
    for i in range(30):
        d[i] = max(d[i], 1)
    return O.dhtgen(ll, d)


def own_table(b, h):
    tok, nt = O.lz77(b, h)
    ll, d = O.counts(tok, nt)
    return O.dhtgen(ll, d)


def dht_array(tables):
    arr = np.zeros(len(tables), pkg.DHT_DTYPE)
    for i, (bits, n) in enumerate(tables):
        arr["dhtlen"][i] = n
        arr["dht"][i, :len(bits)] = np.frombuffer(bits, np.uint8)
    return arr


def run(eng, fc, blocks, hists, tables=None, use=None, check=None):
    """one batch through the engine -> (results, output rows)"""
    import torch
    host = np.zeros((len(blocks), STRIDE_IN), np.uint8)
    for i, b in enumerate(blocks):
        host[i, :len(b)] = np.frombuffer(b, np.uint8)
    src = torch.from_numpy(host).to(eng.dev)
    dst = torch.zeros((len(blocks), STRIDE_OUT), dtype=torch.uint8, device=eng.dev)
    jobs = eng.jobs_strided(src, STRIDE_IN, np.array([len(b) for b in blocks], np.uint32), dst, STRIDE_OUT, STRIDE_OUT,
                            hist_len=np.array(hists, np.uint32), dht_index=None if use is None else np.array(use, np.uint32))
    old = os.environ.get("NXZ_ENCODE_CHECK")
    if check is not None:
        os.environ["NXZ_ENCODE_CHECK"] = check
    try:
        dht = eng.to_device(dht_array(tables)) if tables else None
        res, _ = eng.compress(fc, jobs, len(blocks), dht=dht, ntables=len(tables) if tables else 0)
        r = eng.results_to_host(res).copy()
    finally:
        if check is not None:
            if old is None:
                os.environ.pop("NXZ_ENCODE_CHECK", None)
            else:
                os.environ["NXZ_ENCODE_CHECK"] = old
    return r, dst.cpu().numpy()


def same_as(r, out, i, exp, bits, b, h):
    assert r["cc"][i] in (0, 64), (i, r["cc"][i])
    assert r["cc"][i] == (64 if len(exp) > len(b) else 0), (i, r["cc"][i], len(exp), len(b))
    assert r["tpbc"][i] == len(exp) and r["tebc"][i] == bits % 8, (i, r["tpbc"][i], len(exp))
    assert out[i, :len(exp)].tobytes() == exp, i
    dz = zlib.decompressobj(-15, zdict=b[:h]) if h else zlib.decompressobj(-15)
    assert dz.decompress(exp) == b[h:] and dz.eof, i


def through_all_forms(eng, blocks, hists=None):
    hists = hists or [0] * len(blocks)
    resume = 0x08                                   # (the function codes that take a history)
    # the fixed code, with symbol counts: encode_kernel<false>
    r, out = run(eng, pkg.FC_COMPRESS_FHT_COUNT | resume, blocks, hists)
    for i, (b, h) in enumerate(zip(blocks, hists)):
        exp, bits = O.deflate_fixed(b, hist=h)
        same_as(r, out, i, exp, bits, b, h)
    # a caller's table: the checked form
    uni = universal_table(blocks, hists)
    r, out = run(eng, pkg.FC_COMPRESS_DHT_COUNT | resume, blocks, hists, tables=[uni], use=[0] * len(blocks))
    for i, (b, h) in enumerate(zip(blocks, hists)):
        exp, bits = O.deflate_dynamic(b, uni[0], uni[1], hist=h)
        assert exp is not None
        same_as(r, out, i, exp, bits, b, h)
    # the device's table: the default form, and the checked one
    got = {}
    for chk in ("0", "1"):
        r, out = run(eng, pkg.FC_COMPRESS_DHTGEN_COUNT | resume, blocks, hists, check=chk)
        got[chk] = (r, out)
        for i, (b, h) in enumerate(zip(blocks, hists)):
            t = own_table(b, h)
            exp, bits = O.deflate_dynamic(b, t[0], t[1], hist=h)
            same_as(r, out, i, exp, bits, b, h)
    (ra, oa), (rb, ob) = got["0"], got["1"]
    for f in ("cc", "tpbc", "tebc"):
        assert (ra[f] == rb[f]).all(), f
    for i in range(len(blocks)):
        assert oa[i, :ra["tpbc"][i]].tobytes() == ob[i, :ra["tpbc"][i]].tobytes(), i


# ---------------------------------------------------------------------------
# tests
# ---------------------------------------------------------------------------
def test_record_counts_of_a_round_across_the_staging_passes(eng):
    block = word_rounds(WORDS, WORDS_SEED)
    dense = small_alphabet(3, 65536, 6)
    counts = round_counts(block)
    print("records per round:", counts, "dense data:", max(round_counts(dense)))
    for k in ROUND_COUNTS_WANTED:
        assert k in counts, (k, counts)
    assert max(round_counts(dense)) > 256                 # two passes on data that is nobody's construction
    through_all_forms(eng, [block, dense])


def test_two_matches_in_one_quad(eng):
    """a 3-byte match at the first position of a quad and the next match at its fourth, in a lane's first quad and in its second"""
    blocks = [small_alphabet(1, 65536, 4), small_alphabet(167, 65536, 3)]
    first = second = 0
    for b in blocks:
        starts = {p: ln for p, ln, _ in match_tokens(b)}
        for p, ln in starts.items():
            if ln == 3 and p % 4 == 0 and p + 3 in starts:
                if p % 8 == 0:
                    first += 1
                else:
                    second += 1
    print("quads with two matches: first of a lane %d, second %d" % (first, second))
    assert first >= 40 and second >= 1
    through_all_forms(eng, blocks)


def test_length_and_distance_edges(eng):
    block, want = edge_block()
    toks = match_tokens(block)
    have = {(ln, d) for _, ln, d in toks}
    missing = [w for w in want if w not in have]
    print("strings not matched as laid out:", missing)
    lens = {ln for _, ln, _ in toks}
    dists = {d for _, _, d in toks}
    # every length where the number of extra bits changes, both sides, and the 258 that has a symbol of its own
    for ln in (4, 10, 11, 18, 19, 34, 35, 66, 67, 130, 131, 257, 258):
        assert ln in lens, ln
    for d in (1, 2, 3, 4, 5, 4096, 4097, 32768):
        assert d in dists, d
    assert (258, 1) in have
    through_all_forms(eng, [block])


def test_sizes_and_a_history(eng):
    dense = small_alphabet(9, 65536, 6)
    blocks = [dense[:n] for n in (0, 1, 7, 8, 9, 2047, 2048, 2049, 65536)]
    hists = [0] * len(blocks)
    # a job with a history: its first matches reach back into it
    blocks.append(dense[:4096] + dense[1000:4000] + small_alphabet(10, 3000, 6))
    hists.append(4096)
    assert any(d > p for p, _, d in match_tokens(blocks[-1], 4096))
    through_all_forms(eng, blocks, hists)


def test_a_table_without_a_needed_symbol_answers_missing_code(eng):
    """a caller's table that lacks a length, a distance or a literal symbol the block uses: NXZ_CC_MISSING_CODE, as the
    oracle refuses the block; the same symbols taken from a table of a block that does not use them: no complaint"""
    block = small_alphabet(4, 30000, 6) + bytes(range(64, 128)) * 4
    tok, nt = O.lz77(block)
    tables, expect = [], []

    def table_without(ll_zero=(), d_zero=()):
        ll, d = O.counts(tok, nt)
        for i in ll_zero:
            assert ll[i] > 0
            ll[i] = 0
        for i in d_zero:
            assert d[i] > 0
            d[i] = 0
        return O.dhtgen(ll, d)
    ll, d = O.counts(tok, nt)
    used_len = max(i for i in range(257, 286) if ll[i])
    used_dist = max(i for i in range(30) if d[i])
    used_lit = 100
    tables.append(table_without())                              # exact: every unused symbol is without a code
    tables.append(table_without(ll_zero=[used_len]))
    tables.append(table_without(d_zero=[used_dist]))
    tables.append(table_without(ll_zero=[used_lit]))
    # a block that uses none of the three, under each of the tables
    plain = small_alphabet(4, 30000, 6)[:2000]
    ptok, pnt = O.lz77(plain)
    pll, pd = O.counts(ptok, pnt)
    blocks = [block] * 4 + [plain] * 4
    use = [0, 1, 2, 3, 0, 1, 2, 3]
    r, out = run(eng, pkg.FC_COMPRESS_DHT_COUNT, blocks, [0] * 8, tables=tables, use=use)
    verdicts = []
    for i, (b, u) in enumerate(zip(blocks, use)):
        exp, bits = O.deflate_dynamic(b, tables[u][0], tables[u][1])
        verdicts.append(exp is None)
        if exp is None:
            assert r["cc"][i] == MISSING_CODE, (i, r["cc"][i])
        else:
            assert r["cc"][i] != MISSING_CODE, i
            same_as(r, out, i, exp, bits, b, 0)
    print("oracle refuses:", verdicts)
    assert verdicts[:4] == [False, True, True, True]
    assert not pll[used_len] and not pll[used_lit], "the plain block must not use the symbols taken away"
    assert verdicts[4:6] == [False, False] and not verdicts[7]
