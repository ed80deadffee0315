"""Seeded inputs that sit on the regime switches and numeric edges of oracle/nxz_lz77.c (steps 3, 3b, 3c, 4 and 5 of its
header).  Every generator is deterministic and returns cases (name, data, hist_len): data[:hist_len] is history, the rest
the block; hist_len + block <= 65536, one sub-block each.  META[name] says what a case was built to show (positions,
expected outcome) for tests/test_lz77_cases_host.py, which checks on the CPU that the set does what it claims.

Two kinds of ground keep a planted string's bucket entries alive: a fill of one byte value (positions deep inside a run
take no part in the hash table, so nothing is evicted; after a first tile of few tokens the later tiles run WITHOUT second
entries) and `bin-hard` text (a first tile of >= 3072 tokens with bytes >= 0x80: the later tiles keep second entries and
the lazy step).  Planted strings are fenced by delimiter bytes that occur nowhere else, so that a match starts where the
string starts.
"""
import functools
import random

import oracle_lib as O
from datagen import ALPHABET33

TILE, PIECE, CHUNK = 16384, 512, 64
HARD33 = bytes(range(0x80, 0xA1))
assert len(HARD33) == 33
META = {}


def _rng(*key):
    return random.Random("lz77_cases/" + "/".join(map(str, key)))


def _copy_mix(buf, n, rnd, alphabet):
    """lz-style tail: copies of 4..39 bytes from up to 40000 back (beyond 32768 no match can follow them), now and then
    a literal in between"""
    while len(buf) < n:
        if rnd.random() < 0.25:
            buf.append(rnd.choice(alphabet))
        dist = rnd.randrange(2, min(40000, len(buf)) + 1)
        for _ in range(rnd.randrange(4, 40)):
            buf.append(buf[-dist])
    del buf[n:]
    return buf


def _hard(n, seed, alphabet=HARD33):
    rnd = _rng("hard", n, seed, alphabet[0])
    buf = bytearray(rnd.choices(alphabet, k=min(n, 20000 if n >= 32768 else 5000)))
    return bytes(_copy_mix(buf, n, rnd, alphabet))


def bin_hard():
    """not text, >= 3072 tokens in the first tile: the one regime with second entries and the lazy step live in tiles 1..3"""
    out = [("bin-hard/65536/s%d" % s, _hard(65536, s), 0) for s in range(4)]
    out += [("bin-hard/%d" % n, _hard(n, 9), 0) for n in (49152, TILE + PIECE + 1, TILE + 16, 32768)]
    return out


def _threshold_block(L, alphabet_base, run_byte):
    """first tile: L random bytes of a 128-symbol alphabet, then one byte value up to 16384; second tile: a copy mix"""
    pool = bytes(alphabet_base + b for b in _rng("thr-pool", alphabet_base).choices(range(128), k=4096))
    buf = bytearray(pool[:L] + bytes([run_byte]) * (TILE - L))
    return bytes(_copy_mix(buf, 2 * TILE, _rng("thr-mix", alphabet_base), HARD33 if alphabet_base else ALPHABET33))


@functools.lru_cache(maxsize=None)
def token_threshold():
    """first-tile token counts of exactly 3071, 3072, 3073 (step 3b), over bytes >= 0x80 (use_second flips) and over a 7-bit
    alphabet (text: lazy_max flips, step 3c).  L is found by search with the oracle's tap."""
    out = []
    for base, run_byte, tag in ((0x80, 0xEE, "high"), (0x00, 0x41, "text")):
        want, L = {3071, 3072, 3073}, 2900
        while want and L < 3300:
            data = _threshold_block(L, base, run_byte)
            t0 = O.lz77_regime(data)[2][0][1]
            if t0 in want:
                want.discard(t0)
                name = "threshold/%s/%d" % (tag, t0)
                META[name] = dict(tok0=t0, L=L)
                out.append((name, data, 0))
            L += 1
        assert not want, (tag, want)
    return tuple(out)


def _with_high(data, k, lo, hi, rnd):
    b = bytearray(data)
    for p in rnd.sample(range(lo, hi), k):
        b[p] |= 0x80
    return bytes(b)


def text_threshold():
    """ASCII lz-style blocks with a hard first tile and exactly k bytes >= 0x80 in it: 1023 / 1024 are the two sides of
    `high * 16 < 16384`; 963 / 964 and 1092 / 1093 are where a divisor of 17 or 15 would switch.  n < 16384: t0n = n."""
    out = []
    for n, ks in ((2 * TILE, (1023, 1024, 963, 964, 1092, 1093)), (20000, (1023, 1024)), (8000, (499, 500))):
        base = _hard(n, 3, ALPHABET33)
        for k in ks:
            name = "text-threshold/%d/%d" % (n, k)
            META[name] = dict(high=k, t0n=min(n, TILE))
            out.append((name, _with_high(base, k, 0, min(n, TILE), _rng("high", n, k)), 0))
    return out


class _Ground:
    """a buffer over which strings are planted between unique delimiter bytes"""

    def __init__(self, base, avoid=b""):
        self.b = bytearray(base)
        used = set(base) | set(avoid)
        self.delims = [d for d in range(255, 0, -1) if d not in used]

    def plant(self, pos, s):
        assert pos >= 1 and pos + len(s) + 1 <= len(self.b)
        self.b[pos - 1] = self.delims.pop()
        self.b[pos:pos + len(s)] = s
        self.b[pos + len(s)] = self.delims.pop()
        return pos

    def bytes(self):
        return bytes(self.b)


def _payload(rnd, k):
    """k random bytes of 0x20 .. 0x7f (no ground and no delimiter is among them)"""
    return bytes(rnd.randrange(0x20, 0x80) for _ in range(k))


def window_edge():
    """a 24-byte marker at p and at p + d, d = 32767, 32768 (a match at that distance) and 32769 (none), inside the block and
    with the first marker in a 32768-byte history; periods 1, 2, 3, 4 and 8 for the smallest distances"""
    out = []
    for where, hist in (("block", 0), ("history", 32768)):
        for d in (32767, 32768, 32769):
            rnd = _rng("window", where, d)
            n = hist + 32768 if hist else 100 + d + 24 + 40
            g = _Ground(bytes([0x11]) * n)
            m = _payload(rnd, 24)
            g.plant(100, m)
            g.plant(100 + d, m)
            name = "window/%s/%d" % (where, d)
            META[name] = dict(marker=100 + d - hist, dist=d)
            out.append((name, g.bytes(), hist))
    for period in (1, 2, 3, 4, 8):
        unit = _payload(_rng("period", period), period)
        n = TILE + 700
        out.append(("window/period/%d" % period, (unit * (n // period + 1))[:n], 0))
    return out


def lazy_edge():
    """U (k bytes) + a foreign byte and U[1:] + V earlier, U + V later: the match of k bytes at U gives way to the longer one
    a byte on iff k < LAZY_MAX = 32.  Once in tile 0 over a fill, once in tile 1 of a bin-hard block (lazy stays on)."""
    out = []
    for k in (30, 31, 32, 33):
        rnd = _rng("lazy", k)
        U, V = _payload(rnd, k), _payload(rnd, 12)
        g = _Ground(bytes([0x11]) * 1200)
        g.plant(100, U + b"\x01")
        g.plant(300, U[1:] + V)
        at = g.plant(700, U + V)
        name = "lazy/tile0/%d" % k
        META[name] = dict(at=at, k=k)
        out.append((name, g.bytes(), 0))
        g = _Ground(_hard(2 * TILE, 20 + k), avoid=U + V)
        g.plant(TILE - 300, U + b"\x01")
        g.plant(TILE - 200, U[1:] + V)
        at = g.plant(TILE + 100, U + V)
        name = "lazy/tile1/%d" % k
        META[name] = dict(at=at, k=k)
        out.append((name, g.bytes(), 0))
    return out


def tile_cut():
    """a 64-byte string seen at 50 (or 30000 back) comes again `64 - rem` bytes in front of a tile end (rem = 61: a 3-byte match is left; 62:
    it is dropped), in front of the sub-block's end, and in front of 65536; blocks whose last tile is 1 .. 5 bytes"""
    out = []

    def case(name, n, at, **meta):
        g = _Ground(bytes([0x11]) * n)
        s = _payload(_rng("cut", name), 64)
        g.plant(max(50, at - 30000), s)
        if at + 64 < n:
            g.plant(at, s)
        else:                                                 # the block ends inside the string
            g.b[at - 1] = g.delims.pop()
            g.b[at:] = s[:n - at]
        META[name] = dict(at=at, **meta)
        out.append((name, g.bytes(), 0))
    for rem in (0, 1, 2, 3, 4, 61, 62, 63):
        case("cut/tile/%d" % rem, TILE + 200, TILE - 64 + rem, left=64 - rem)
    for rem in (1, 2, 3, 4, 5):
        case("cut/last-tile/%d" % rem, TILE + rem, TILE - 30, left=30)
    for n in (20000, 65536):
        for left in (5, 4, 3, 2):
            case("cut/end/%d/%d" % (n, left), n, n - left, left=left)
    return out


def length_edge():
    """repeats of 257, 258, 259, 516, 517 bytes at a distance > 1 and at distance 1 (runs); a bucket candidate exactly as long
    as the run where both stand: `l1 >= len` takes distance 1"""
    out = []
    for L in (257, 258, 259, 516, 517):
        rnd = _rng("length", L)
        s = _payload(rnd, L)
        g = _Ground(bytes([0x11]) * (2 * L + 400))
        g.plant(50, s)
        at = g.plant(50 + L + 100, s)
        name = "length/far/%d" % L
        META[name] = dict(at=at, L=L)
        out.append((name, g.bytes(), 0))
        g = _Ground(bytes([0x11]) * (L + 300))
        at = g.plant(100, bytes([0x42]) * (L + 1))
        name = "length/run/%d" % L
        META[name] = dict(at=at, L=L)
        out.append((name, g.bytes(), 0))
    for m in (4, 5):
        # "x a^m y" earlier; later "P a" + a^m: the match of P + a ends on the second a of the run, where the run's m
        # bytes at distance 1 tie with the earlier a^m
        rnd = _rng("tie", m)
        P = _payload(rnd, 8)
        g = _Ground(bytes([0x11]) * 900)
        g.plant(100, b"a" * m)
        g.plant(200, P + b"a")
        at = g.plant(CHUNK * 10 + 32 - 9, P + b"a" + b"a" * m) + 9
        name = "length/tie/%d" % m
        META[name] = dict(at=at, L=m)
        out.append((name, g.bytes(), 0))
    return out


def run_edge():
    """runs of 10 .. 13 equal bytes in front of a 4-gram seen before: the run's last `aaaa` position is deep in the run from 12
    on (neither inserted nor looked up).  insert: "a^m G T" early -- at the very start behind histories of 0, 4, 8, 16 bytes, so
    that r - 8 falls in front of the buffer, into the history, or on a tile seam --, "aaaa G T" later finds it or does not;
    lookup: a match ends four bytes in front of the run's end, where "aaaa G T" seen earlier is looked up or is not."""
    out = []
    for m in (10, 11, 12, 13):
        rnd = _rng("run", m)
        G, T, P = _payload(rnd, 4), _payload(rnd, 8), _payload(rnd, 8)
        run = b"a" * m
        for hist in (0, 4, 8, 16):
            g = _Ground(bytes([0x11]) * 700, avoid=b"a")
            g.b[:m + 12] = run + G + T                       # the run starts the buffer
            g.b[m + 12] = g.delims.pop()
            at = g.plant(300 + hist, b"aaaa" + G + T)
            name = "run/insert/h%d/%d" % (hist, m)
            META[name] = dict(at=at - hist, deep=m >= 12, far=at - (m - 4))
            out.append((name, g.bytes(), hist))
        g = _Ground(bytes([0x11]) * (TILE + 700), avoid=b"a")
        s = g.plant(TILE - 6, run + G + T)
        at = g.plant(TILE + 400, b"aaaa" + G + T)
        name = "run/insert/tile/%d" % m
        META[name] = dict(at=at, deep=m >= 12, far=at - (s + m - 4))
        out.append((name, g.bytes(), 0))
        g = _Ground(bytes([0x11]) * 900, avoid=b"a")
        g.plant(100, P + b"a" * (m - 4))
        e = g.plant(200, b"aaaa" + G + T)
        s = g.plant(CHUNK * 10 + 8 - 8, P + run + G + T) + 8  # the run at offset 8 of its chunk
        name = "run/lookup/%d" % m
        META[name] = dict(at=s + m - 4, deep=m >= 12, far=s + m - 4 - e)
        out.append((name, g.bytes(), 0))
    return out


def piece_lag():
    """X (16 bytes) at p0, X[:5] + junk at p1 (the newest entry, 5 bytes agree), X again at p2: p0 is taken iff it is a second
    entry by then -- the notes of piece c are second entries from piece c + 2 on, all notes at a tile's end; in the later tiles
    only where the first tile was hard."""
    out = []

    def case(name, n, p0, p1, p2, visible, ground=None):
        rnd = _rng("piece", name)
        X = _payload(rnd, 16)
        g = _Ground(ground or bytes([0x11]) * n, avoid=X)
        g.plant(p0, X)
        g.plant(p1, X[:5] + bytes(0x10 + (c & 0xf) for c in rnd.randbytes(11)))
        g.plant(p2, X)
        META[name] = dict(at=p2, visible=visible, far=p2 - p0, near=p2 - p1)
        out.append((name, g.bytes(), 0))
    p1 = 3 * PIECE - 30
    for delta in (60, 500, 520, 1030, 1500):
        vis = (p1 + delta) // PIECE - p1 // PIECE >= 2
        case("piece/tile0/%d" % delta, 4000, 100, p1, p1 + delta, vis)
    p1 = TILE - 30                                            # astride the tile boundary: all notes are in at its end
    for delta in (60, 520):
        case("piece/tile-seam/fill/%d" % delta, TILE + 1000, p1 - 200, p1, p1 + delta, False)     # easy tile 0: no second entries
        case("piece/tile-seam/hard/%d" % delta, 0, p1 - 200, p1, p1 + delta, True, ground=_hard(2 * TILE, 40 + delta))
    for delta in (60, 250):                                   # p1 in the last, shorter piece of a ragged tile
        n = TILE + PIECE + 300
        case("piece/ragged/%d" % delta, 0, TILE + PIECE - 150, TILE + PIECE + 10, TILE + PIECE + 10 + delta, False,
             ground=_hard(n, 50 + delta))
    return out


HISTORIES = (0, 1, 15, 16, 17, 4095, 32767, 32768)


def history():
    """bin-hard and text bodies of two tiles behind histories of every length class; the body copies from its history"""
    out = []
    for tag, alphabet in (("bin", HARD33), ("text", ALPHABET33)):
        for h in HISTORIES:
            rnd = _rng("history", tag, h)
            buf = bytearray(rnd.choices(alphabet, k=h))
            while len(buf) < h + 12000:                       # a hard first tile that still refers to the history
                buf += bytes(rnd.choices(alphabet, k=48))
                if h >= 4:
                    src = rnd.randrange(0, h)
                    buf += buf[src:src + rnd.randrange(8, 21)]
            _copy_mix(buf, h + 2 * TILE, rnd, alphabet)
            out.append(("history/%s/%d" % (tag, h), bytes(buf), h))
    return out


FAMILIES = dict(bin_hard=bin_hard, token_threshold=token_threshold, text_threshold=text_threshold, window_edge=window_edge,
                lazy_edge=lazy_edge, tile_cut=tile_cut, length_edge=length_edge, run_edge=run_edge, piece_lag=piece_lag,
                history=history)


@functools.lru_cache(maxsize=None)
def all_cases():
    """every family's cases, in a fixed order; names are unique"""
    out = [c for f in FAMILIES.values() for c in f()]
    assert len({c[0] for c in out}) == len(out)
    assert all(len(d) <= 65536 and h <= 32768 for _, d, h in out)
    return tuple(out)


def family(name):
    return [c for c in all_cases() if c[0].startswith(name)]


def events(tok, nt):
    """a token stream as (position, length, distance) with (p, 1, 0) for a literal"""
    out, p = [], 0
    for i in range(nt):
        t = tok[i]
        if t & O.TOK_MATCH:
            out.append((p, (t & 0xff) + 3, ((t >> 8) & 0x7fff) + 1))
            p += (t & 0xff) + 3
        else:
            out.append((p, 1, 0))
            p += 1
    return out
