"""Streams for the one-pass index build (nxz_batch_checkpoint_build) that zlib never writes: a helper, not a test.

zlib keeps its distances at or below 32 506, so the far edge of a 32 KiB ring -- a match at distance 32 768, which reads the very
byte it is about to replace -- needs hand-built streams.  encode() is a small fixed-Huffman (BTYPE 1) encoder driven by a token list,
stored() writes stored blocks; streams() returns two raw deflate streams with their plain bytes, each checked on the CPU against
zlib's inflate and against the replay of its own tokens:
  far_fixed    32 768 + 5 literals, then at least 4000 seeded tokens: literals and matches with len in {3, 4, 17, 258} and dist in
               {1, 2, len - 1, len, 16, 32 767, 32 768}; in front of every multiple of 32 768 of output a match is placed so that it
               straddles it
  far_stored   stored blocks of 65 535, 1, 0 and 65 535 bytes (two of them cross a multiple of 32 768), then a fixed block whose
               distance-32 768 matches reach into the stored bytes"""
import random
import zlib

WINDOW = 32768
FMT_RAW = 0
LENS = (3, 4, 17, 258)

LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEXT = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
DEXT = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]


class BitWriter:
    def __init__(self):
        self.chunks, self.acc, self.n = [], 0, 0

    def bits(self, v, n):                            # n bits of v, LSB first
        self.acc |= v << self.n
        self.n += n
        if self.n >= 4096:
            k = self.n // 8
            self.chunks.append((self.acc & ((1 << 8 * k) - 1)).to_bytes(k, "little"))
            self.acc >>= 8 * k
            self.n -= 8 * k

    def code(self, c, n):                            # a Huffman code: its first bit first
        self.bits(int(format(c, "0%db" % n)[::-1], 2), n)

    def align(self):
        self.bits(0, (-self.n) & 7)

    def bytes_(self, data):
        assert self.n % 8 == 0
        self.bits(int.from_bytes(data, "little"), 8 * len(data))

    def done(self):
        self.align()
        return b"".join(self.chunks) + self.acc.to_bytes(self.n // 8, "little")


def litlen(w, s):
    if s < 144:
        w.code(0x30 + s, 8)
    elif s < 256:
        w.code(0x190 + s - 144, 9)
    elif s < 280:
        w.code(s - 256, 7)
    else:
        w.code(0xc0 + s - 280, 8)


def encode(w, tokens, final):
    """one fixed block: tokens are ("L", byte) and ("M", len, dist)"""
    w.bits(final | 1 << 1, 3)
    for t in tokens:
        if t[0] == "L":
            litlen(w, t[1])
            continue
        _, n, d = t
        ls = max(i for i in range(29) if LBASE[i] <= n and (i == 28 or n < 258))
        litlen(w, 257 + ls)
        w.bits(n - LBASE[ls], LEXT[ls])
        ds = max(i for i in range(30) if DBASE[i] <= d)
        w.code(ds, 5)
        w.bits(d - DBASE[ds], DEXT[ds])
    litlen(w, 256)


def stored(w, data, final):
    assert len(data) <= 65535
    w.bits(final, 3)
    w.align()
    w.bits(len(data) | (len(data) ^ 0xffff) << 16, 32)
    w.bytes_(data)


def replay(out, tokens):
    """the tokens applied to bytearray out; -> [(u, len, dist)] of the matches"""
    matches = []
    for t in tokens:
        if t[0] == "L":
            out.append(t[1])
            continue
        _, n, d = t
        u = len(out)
        assert 1 <= d <= min(u, WINDOW) and 3 <= n <= 258
        matches.append((u, n, d))
        for i in range(n):
            out.append(out[u - d + i])
    return matches


def crosses(a, n):
    """do the n bytes from output byte a on lie on both sides of a multiple of 32 768?"""
    return n > 0 and a // WINDOW != (a + n - 1) // WINDOW


def far_fixed_tokens(rnd):
    tokens = [("L", rnd.randrange(256)) for _ in range(WINDOW + 5)]
    u, forced = WINDOW + 5, 0
    rest = 0
    while rest < 4000 or u < 170 << 10:
        gap = -u % WINDOW                            # bytes up to the next multiple of 32 768
        if 1 <= gap <= 257:                          # a match of 258 bytes lies across it: far, self-feeding and just short of far in turn
            t = ("M", 258, (WINDOW, 1, WINDOW - 1, 2)[forced % 4])
            forced += 1
        elif rnd.random() < 0.45:
            t = ("L", rnd.randrange(256))
        else:
            n = rnd.choice(LENS if rnd.random() < 0.3 else LENS[:3])
            t = ("M", n, rnd.choice((1, 2, n - 1, n, 16, WINDOW - 1, WINDOW)))
        tokens.append(t)
        u += 1 if t[0] == "L" else t[1]
        rest += 1
    return tokens, rest


_STREAMS = None


def streams():
    """-> [(name, FMT_RAW, stream, plain)]"""
    global _STREAMS
    if _STREAMS is not None:
        return _STREAMS
    rnd = random.Random(32768)
    seen = set()

    def note(matches):
        for u, n, d in matches:
            if d == WINDOW:
                seen.add("dist 32768")
            if crosses(u, n):
                seen.add("target across")
                if d < n:
                    seen.add("self-feeding across")
            if crosses(u - d, min(n, d)):
                seen.add("source across")

    # far_fixed
    tokens, rest = far_fixed_tokens(rnd)
    w = BitWriter()
    encode(w, tokens, 1)
    fixed = w.done()
    plain = bytearray()
    m = replay(plain, tokens)
    note(m)
    assert rest >= 4000 and len(plain) >= 100 << 10
    assert {n for _, n, _ in m} == set(LENS) and {d for _, _, d in m} >= {1, 2, 16, WINDOW - 1, WINDOW}
    out = [("far_fixed", FMT_RAW, fixed, bytes(plain))]

    # far_stored
    runs = [bytes(rnd.randrange(256) for _ in range(n)) for n in (65535, 1, 0, 65535)]
    w = BitWriter()
    plain = bytearray()
    for r in runs:
        if crosses(len(plain), len(r)):
            seen.add("stored across")
        stored(w, r, 0)
        plain += r
    assert len(plain) == 131071
    tokens = [("M", 258, WINDOW), ("L", 7), ("M", 258, WINDOW), ("M", 3, WINDOW), ("M", 17, WINDOW - 1)]
    tokens += [("M", 258, WINDOW) if k % 3 else ("L", k & 255) for k in range(120)]
    encode(w, tokens, 1)
    note(replay(plain, tokens))
    out.append(("far_stored", FMT_RAW, w.done(), bytes(plain)))

    assert seen == {"dist 32768", "target across", "source across", "self-feeding across", "stored across"}, seen
    for name, _, stream, plain in out:
        d = zlib.decompressobj(-15)
        assert d.decompress(stream) == plain and d.eof and not d.unused_data, name
        assert len(plain) >= 100 << 10, name
    _STREAMS = out
    return out
