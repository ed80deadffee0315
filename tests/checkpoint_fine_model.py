"""The fine checkpoint index of a raw / zlib / gzip stream (nxz_batch_checkpoint_index_fine, include/nxz_engine.h) in plain Python:
the model the device is held to in tests/test_gpu_checkpoints_fine.py, proven itself in tests/test_checkpoint_fine_model_host.py
(its block headers against zlib's Z_BLOCK, its segments against the oracle's resumable decoder).

walk() is a small RFC 1951 token walker: canonical Huffman decode, no window -- it needs the positions and sizes of the tokens, not
their bytes.  It yields, for every byte-making token, the bit of the stream it starts at, the bytes of output in front of it, how
many bytes it makes, and the state of the block it stands in: in_sfbt (0x8 stored, 0xa fixed, 0xc dynamic, | BFINAL), where the
block's table is (tbit, dhtlen; dynamic only) and the stored bytes still to come (rem).  The bytes of a stored block are tokens of
one byte each; they come as ONE record with a count, and index() does their arithmetic.

index() applies the rule: with c the uoff of the last checkpoint, a checkpoint stands in front of the token of n bytes with u bytes
in front of it when u + n > c + span."""
WINDOW = 32768
FMT_RAW, FMT_ZLIB, FMT_GZIP = 0, 1, 2
SPAN_MIN = 258
DHT_MAXSZ = 288

LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEXT = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DEXT = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CLORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


class Bad(Exception):
    """the stream is damaged or ends early"""


def header_len(stream, fmt):
    """bytes of framing in front of the deflate data (gzip: of the first member)"""
    if fmt == FMT_RAW:
        return 0
    if fmt == FMT_ZLIB:
        if len(stream) < 2 or (stream[0] & 15) != 8 or ((stream[0] << 8) | stream[1]) % 31 or stream[1] & 0x20:
            raise Bad("zlib header")
        return 2
    if len(stream) < 10 or stream[0] != 0x1f or stream[1] != 0x8b or stream[2] != 8:
        raise Bad("gzip header")
    flg, p = stream[3], 10
    if flg & 4:
        p += 2 + (stream[p] | stream[p + 1] << 8)
    for bit in (8, 16):
        if flg & bit:
            p = stream.index(0, p) + 1
    if flg & 2:
        p += 2
    if p > len(stream):
        raise Bad("gzip header")
    return p


class Code:
    """a canonical Huffman code: decode(bits as an int, LSB the first bit) -> (symbol, length)"""
    FAST = 9

    def __init__(self, lens, allow_incomplete=False):
        count = [0] * 16
        for l in lens:
            count[l] += 1
        count[0] = 0
        left = 1
        for l in range(1, 16):
            left = 2 * left - count[l]
            if left < 0:
                raise Bad("over-subscribed code")
        if left > 0 and not (allow_incomplete and sum(count) <= 1):
            raise Bad("incomplete code")
        nxt, code = [0] * 16, 0
        for l in range(1, 16):
            code = (code + count[l - 1]) << 1
            nxt[l] = code
        self.fast = [None] * (1 << self.FAST)
        self.slow = {}
        for sym, l in enumerate(lens):
            if not l:
                continue
            c = nxt[l]
            nxt[l] += 1
            rev = int(format(c, "0%db" % l)[::-1], 2)
            if l <= self.FAST:
                for i in range(rev, 1 << self.FAST, 1 << l):
                    self.fast[i] = (sym, l)
            else:
                self.slow[(l, rev)] = sym

    def decode(self, v):
        e = self.fast[v & ((1 << self.FAST) - 1)]
        if e is not None:
            return e
        for l in range(self.FAST + 1, 16):
            s = self.slow.get((l, v & ((1 << l) - 1)))
            if s is not None:
                return s, l
        raise Bad("no such code")


_FIXED = None


def fixed_codes():
    global _FIXED
    if _FIXED is None:
        _FIXED = (Code([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8), Code([5] * 32))
    return _FIXED


def walk(stream, fmt):
    """-> (tokens, headers, end): tokens = [(bit, u, n, count, sfbt, tbit, dhtlen, rem)], count > 1 only for the bytes of a stored
    block (n = 1 each, the first at `bit` with `rem` bytes of the block to come); headers = [(bit, u)] of every block header;
    end = (the bit behind the final end-of-block code, out_len).  Bits count from the first byte of `stream`.  Raises Bad."""
    stream = bytes(stream)
    base = 8 * header_len(stream, fmt)
    total = 8 * len(stream)
    big = int.from_bytes(stream, "little")
    CH = 1 << 15                                     # bits a chunk of the stream that is looked into at one time holds

    state = {"lo": -1, "v": 0}

    def peek(pos, n):                                # n <= 48 bits at pos; what lies behind the stream reads as zeros
        lo = state["lo"]
        if lo < 0 or pos < lo or pos + n > lo + CH:
            lo = state["lo"] = pos & ~7
            state["v"] = (big >> lo) & ((1 << (CH + 64)) - 1)
        return (state["v"] >> (pos - lo)) & ((1 << n) - 1)

    def need(pos, n):
        if pos + n > total:
            raise Bad("the source ends early")

    tokens, headers = [], []
    pos, u = base, 0
    while True:
        headers.append((pos, u))
        need(pos, 3)
        h = peek(pos, 3)
        bfinal, btype = h & 1, h >> 1
        pos += 3
        if btype == 0:
            pos = (pos + 7) & ~7
            need(pos, 32)
            w = peek(pos, 32)
            if (w ^ (w >> 16)) & 0xffff != 0xffff:
                raise Bad("stored length")
            pos += 32
            rem = w & 0xffff
            need(pos, 8 * rem)
            if rem:
                tokens.append((pos, u, 1, rem, 0x8 | bfinal, 0, 0, rem))
            pos += 8 * rem
            u += rem
        elif btype == 3:
            raise Bad("block type 3")
        else:
            tbit = dhtlen = 0
            if btype == 1:
                lit, dist = fixed_codes()
            else:
                tbit = pos
                need(pos, 14)
                hlit, hdist, hclen = peek(pos, 5) + 257, peek(pos + 5, 5) + 1, peek(pos + 10, 4) + 4
                pos += 14
                if hlit > 286 or hdist > 30:
                    raise Bad("too many codes")
                need(pos, 3 * hclen)
                cl = [0] * 19
                for i in range(hclen):
                    cl[CLORDER[i]] = peek(pos + 3 * i, 3)
                pos += 3 * hclen
                clc = Code(cl)
                lens = []
                while len(lens) < hlit + hdist:
                    need(pos, 1)
                    s, l = clc.decode(peek(pos, 15))
                    need(pos, l)
                    pos += l
                    if s < 16:
                        lens.append(s)
                        continue
                    xb, xbase = ((2, 3), (3, 3), (7, 11))[s - 16]
                    need(pos, xb)
                    rep = xbase + peek(pos, xb)
                    pos += xb
                    if s == 16 and not lens:
                        raise Bad("repeat without a length")
                    lens += [lens[-1] if s == 16 else 0] * rep
                if len(lens) > hlit + hdist:
                    raise Bad("repeat runs over")
                if lens[256] == 0:
                    raise Bad("no end-of-block code")
                lit, dist = Code(lens[:hlit]), Code(lens[hlit:], allow_incomplete=True)
                dhtlen = pos - tbit
            sfbt = (0xa if btype == 1 else 0xc) | bfinal
            while True:
                need(pos, 1)
                start = pos
                s, l = lit.decode(peek(pos, 15))
                need(pos, l)
                pos += l
                if s < 256:
                    tokens.append((start, u, 1, 1, sfbt, tbit, dhtlen, 0))
                    u += 1
                elif s == 256:
                    break
                else:
                    s -= 257
                    if s >= 29:
                        raise Bad("length symbol")
                    need(pos, LEXT[s])
                    n = LBASE[s] + peek(pos, LEXT[s])
                    pos += LEXT[s]
                    need(pos, 1)
                    d, l = dist.decode(peek(pos, 15))
                    need(pos, l)
                    pos += l
                    if d >= 30:
                        raise Bad("distance symbol")
                    need(pos, DEXT[d])
                    back = ((2 + (d & 1)) << DEXT[d]) + 1 + peek(pos, DEXT[d]) if d >= 4 else d + 1
                    pos += DEXT[d]
                    if back > u:
                        raise Bad("distance reaches in front of the output")
                    tokens.append((start, u, n, 1, sfbt, tbit, dhtlen, 0))
                    u += n
        if bfinal:
            return tokens, headers, (pos, u)


_WALKS = {}


def walk_cached(stream, fmt):
    key = (bytes(stream), fmt)
    if key not in _WALKS:
        try:
            _WALKS[key] = walk(stream, fmt)
        except (Bad, ValueError, IndexError):
            _WALKS[key] = None
    return _WALKS[key]


def state_entry(sfbt, rem, tbit, dhtlen):
    """(tbit, resume, dhtlen) as nxz_checkpoint_state_t holds them"""
    if (sfbt & 0xe) == 0x8:
        return (0, rem | sfbt << 16, 0)
    if (sfbt & 0xe) == 0xc:
        return (tbit, sfbt << 16, dhtlen)
    return (0, sfbt << 16, 0)


def index(stream, fmt, span):
    """-> None for a stream that fails or does not reach the end of its final block, else a dict: cbit / uoff / state (count + 1
    entries, the sentinel last; a state is (tbit, resume, dhtlen)), count, out_len, hdr_len."""
    assert span >= SPAN_MIN
    w = walk_cached(stream, fmt)
    if w is None:
        return None
    tokens, headers, end = w
    if end[1] > 0xffffffff:
        return None
    cbit, uoff, state = [headers[0][0]], [0], [(0, 0, 0)]
    c = 0
    for bit, u, n, count, sfbt, tbit, dhtlen, rem in tokens:
        if count == 1:
            if u + n > c + span:
                cbit.append(bit); uoff.append(u); state.append(state_entry(sfbt, 0, tbit, dhtlen))
                c = u
            continue
        while u + count > c + span:                  # byte i of the run is the first that does not fit
            i = c + span - u
            cbit.append(bit + 8 * i); uoff.append(u + i); state.append(state_entry(sfbt, rem - i, 0, 0))
            c = u + i
    return {"cbit": cbit + [end[0]], "uoff": uoff + [end[1]], "state": state + [(0, 0, 0)], "count": len(cbit), "out_len": end[1],
            "hdr_len": headers[0][0] // 8}


def table_bits(stream, tbit, dhtlen):
    """bits [tbit, tbit + dhtlen) of the stream shifted to bit 0, as the bytes of a table slot (zeros behind)"""
    v = (int.from_bytes(bytes(stream), "little") >> tbit) & ((1 << dhtlen) - 1)
    return v.to_bytes((dhtlen + 7) // 8, "little")


def segment(idx, k):
    """segment k of an index: (first source byte, end source byte, in_subc, window length, output bytes, in_sfbt, rem, tbit, dhtlen)"""
    c0, c1, u0, u1 = idx["cbit"][k], idx["cbit"][k + 1], idx["uoff"][k], idx["uoff"][k + 1]
    tbit, resume, dhtlen = idx["state"][k]
    return c0 >> 3, (c1 + 7) >> 3, (8 - (c0 & 7)) & 7, min(u0, WINDOW), u1 - u0, (resume >> 16) & 15, resume & 0xffff, tbit, dhtlen


def broken_states(idx):
    """every kind of broken state entry of a valid fine index -> [(what, index)]"""
    import copy
    n = idx["count"]
    kind = lambda k: (idx["state"][k][1] >> 16) & 0xe
    sto = next((k for k in range(1, n) if kind(k) == 0x8), None)
    dyn = next((k for k in range(1, n) if kind(k) == 0xc), None)
    fix = next((k for k in range(1, n) if kind(k) == 0xa), None)
    out = []

    def put(what, k, **f):
        b = copy.deepcopy(idx)
        t, r, d = b["state"][k]
        b["state"][k] = (f.get("tbit", t), f.get("resume", r), f.get("dhtlen", d))
        if "cbit" in f:
            b["cbit"][k] = f["cbit"]
        out.append((what, b))
    put("entry 0 not at a header", 0, resume=0xa << 16)
    k = fix or dyn or sto
    t, r, d = idx["state"][k]
    put("in_subc in resume", k, resume=r | 1 << 20)
    put("high bits in resume", k, resume=r | 1 << 31)
    for sf in (0x1, 0x7, 0xe, 0xf):
        put("in_sfbt 0x%x" % sf, k, resume=sf << 16, tbit=0, dhtlen=0)
    if sto is not None:
        put("stored without rem", sto, resume=idx["state"][sto][1] & ~0xffff)
        put("stored inside a byte", sto, cbit=idx["cbit"][sto] + 1)
        put("stored with a table", sto, tbit=3, dhtlen=20)
    if fix is not None:
        put("fixed with rem", fix, resume=idx["state"][fix][1] | 5)
        put("fixed with a table", fix, tbit=3, dhtlen=20)
        put("fixed with dhtlen", fix, dhtlen=20)
    if dyn is not None:
        t, r, d = idx["state"][dyn]
        put("dynamic with rem", dyn, resume=r | 1)
        put("dynamic without a table", dyn, dhtlen=0)
        put("table too long", dyn, dhtlen=8 * 288 + 1)
        put("table in front of the stream", dyn, tbit=2)
        put("table behind the checkpoint", dyn, tbit=idx["cbit"][dyn] - d + 1)
        put("table far behind the source", dyn, tbit=(1 << 64) - 8)
    return out



# ---- the streams the fine index is tested on (tests/test_checkpoint_fine_model_host.py on the CPU, tests/test_gpu_checkpoints_fine.py on the device)
_STREAMS = None


def streams():
    """-> [(name, fmt, stream, plain or None)]: 100 - 250 KiB of plain bytes each, the smallest shapes at which each branch of the
    rule can go wrong; plain None: the stream fails (truncated, a damaged table)."""
    global _STREAMS
    if _STREAMS is not None:
        return _STREAMS
    import struct
    import zlib
    import datagen

    def z(data, wbits, level=6, mem=8, strategy=zlib.Z_DEFAULT_STRATEGY):
        c = zlib.compressobj(level, zlib.DEFLATED, wbits, mem, strategy)
        return c.compress(data) + c.flush()

    text = datagen.ALICE_LIKE(120000)
    raw = z(text, -15)
    # gzip with header fields: FEXTRA, FNAME, FCOMMENT and FHCRC in front of the same deflate data
    head = b"\x1f\x8b\x08\x1e" + b"\0\0\0\0\x00\x03" + struct.pack("<H", 6) + b"ab\x02\x00xy" + b"name.txt\0" + b"a comment\0"
    head += struct.pack("<H", zlib.crc32(head) & 0xffff)
    gz = head + raw + struct.pack("<II", zlib.crc32(text), len(text))
    zeros = bytes(200 << 10)
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    tail = c.compress(text[:110000]) + c.flush(zlib.Z_FULL_FLUSH) + c.flush()      # ends with an empty final block
    zl = z(text, 15)
    out = [("alice6_raw", FMT_RAW, raw, text), ("alice6_zlib", FMT_ZLIB, zl, text), ("alice6_gzip_fields", FMT_GZIP, gz, text),
           ("alice1", FMT_ZLIB, z(text, 15, 1), text), ("fixed_one_block", FMT_RAW, z(text, -15, 6, 9, zlib.Z_FIXED), text),
           ("rle_zeros", FMT_ZLIB, z(zeros, 15, 6, 8, zlib.Z_RLE), zeros), ("stored", FMT_ZLIB, z(text + text[:20000], 15, 0), text + text[:20000]),
           ("mem9", FMT_RAW, z(text, -15, 6, 9), text), ("mem1", FMT_GZIP, z(text, 31, 6, 1), text),
           ("empty_final_block", FMT_RAW, tail, text[:110000]),
           ("truncated", FMT_ZLIB, zl[:len(zl) // 2], None)]
    # a flipped bit in the first dynamic table (behind the 2 header bytes, the 3 header bits and HLIT / HDIST / HCLEN) that zlib refuses
    assert (zl[2] >> 1) & 3 == 2
    for bit in range(16 + 3 + 14, 16 + 3 + 14 + 64):
        bad = bytearray(zl)
        bad[bit >> 3] ^= 1 << (bit & 7)
        try:
            zlib.decompress(bytes(bad))
        except zlib.error as e:
            if "code lengths" in str(e) or "lengths set" in str(e):
                out.append(("bad_table", FMT_ZLIB, bytes(bad), None))
                break
    assert out[-1][0] == "bad_table"
    _STREAMS = out
    return out
