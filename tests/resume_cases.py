"""Resume jobs for the inflate routes, held to the CPU oracle alone (no GPU, no engine import).

A case is the SECOND job of a stream that was cut in two: part 1 (the stream's first k bytes) is decoded by the oracle,
and what it reports -- out_sfbt, out_subc, out_rembytecnt, the table of an open dynamic block, the output as history and
its checksums -- becomes the second job's input the way lib/nx_inflate.c:1464-1609 builds it.  The second job's expected
result is the oracle's answer to exactly that input.

The cuts: every byte from 2 in front of each block header to 2 behind the end of its table (behind LEN/NLEN for a stored
block) -- the stops inside headers and tables --, a stored block's first and last bytes, and a seeded sample inside every
block body.  Part 2 is the rest of the stream and 8 trailer bytes, or 1, 2 or 7 bytes, or ends at a second random cut.
The history in front of the source comes in three layouts: 'a' exactly the history, the job's src placed so that the
stream starts at any alignment; 'b' zero bytes in front up to a multiple of 16 and counted in hist_len; 'c' none at all.

tests/test_resume_cases_host.py says what the set must hold; tests/test_gpu_inflate_resume.py runs it on every route."""
import random
import zlib
from collections import namedtuple

import oracle_lib as O
from datagen import make_block

TRAILER = b"12345678"
CAP_MAX = 70000 + 4096              # no stream here holds more plain bytes than 70 000
KINDS = (0xe, 0x8, 0xa, 0xc)

Stream = namedtuple("Stream", "name data comp starts")      # starts: byte offsets of the block headers (all byte aligned)
Case = namedtuple("Case", "stream k m layout shift pad hist part2 subc1 subc sfbt rem dht dhtlen crc1 adler1 cap "
                          "err out tpbc out_sfbt out_subc out_rem out_dht out_dhtlen final_eob pos forced")


def _raw(level=6, strategy=zlib.Z_DEFAULT_STRATEGY):
    return zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)


def _segments(parts):
    """parts: byte strings that each end on a byte boundary (a flush) -> the stream and where each part starts"""
    starts, pos = [], 0
    for p in parts:
        starts.append(pos)
        pos += len(p)
    return b"".join(parts), starts


def streams():
    out = []
    # stored: one block of 65 535 bytes and a final one
    # (what zlib level 0 makes of 70 000 bytes, written out by hand: how zlib sizes its stored blocks differs between versions)
    d = make_block("random", 70000, seed=21)
    c = b"\x00\xff\xff\x00\x00" + d[:65535] + b"\x01" + (4465).to_bytes(2, "little") + (4465 ^ 0xffff).to_bytes(2, "little") + d[65535:]
    out.append(Stream("stored", d, c, [0, 5 + 65535]))
    # stored, with the empty stored block of a Z_SYNC_FLUSH in the middle
    d = make_block("random", 9000, seed=22)
    co = _raw(0)
    a = co.compress(d[:4000]) + co.flush(zlib.Z_SYNC_FLUSH)
    b = co.compress(d[4000:]) + co.flush()
    c, st = _segments([a, b])
    out.append(Stream("stored-sync", d, c, _stored_starts(c)))
    # fixed codes: a block that is not the final one, and the final one
    d = make_block("text33", 20000, seed=23)
    co = _raw(6, zlib.Z_FIXED)
    a = co.compress(d[:11000]) + co.flush(zlib.Z_FULL_FLUSH)
    b = co.compress(d[11000:]) + co.flush()
    c, st = _segments([a, b])
    out.append(Stream("fixed", d, c, st))
    # three dynamic blocks
    d = make_block("alice", 60000, seed=24)
    co = _raw(6)
    parts = [co.compress(d[:20000]) + co.flush(zlib.Z_FULL_FLUSH), co.compress(d[20000:40000]) + co.flush(zlib.Z_FULL_FLUSH),
             co.compress(d[40000:]) + co.flush()]
    c, st = _segments(parts)
    out.append(Stream("dynamic", d, c, st))
    # stored, fixed, dynamic: full-flushed outputs of separate compressors, one behind the other
    ds = [make_block("random", 3000, seed=25), make_block("text33", 6000, seed=26), make_block("alice", 30000, seed=27)]
    co = _raw(0)
    p0 = co.compress(ds[0]) + co.flush(zlib.Z_FULL_FLUSH)
    co = _raw(6, zlib.Z_FIXED)
    p1 = co.compress(ds[1]) + co.flush(zlib.Z_FULL_FLUSH)
    co = _raw(6)
    p2 = co.compress(ds[2]) + co.flush()
    c, st = _segments([p0, p1, p2])
    out.append(Stream("mixed", b"".join(ds), c, st))
    # one block of the oracle's own, with its exact table (HLIT 286 / HDIST 30: the longest table the engine sees)
    d = make_block("alice", 50000, seed=28)
    tok, nt = O.lz77(d)
    ll, dd = O.counts(tok, nt)
    dht, dhtlen = O.dhtgen(ll, dd)
    c, _ = O.deflate_dynamic(d, dht, dhtlen)
    assert c is not None and c[0] & 7 == 0b101              # BFINAL, dynamic
    out.append(Stream("own", d, c, [0]))
    # small blocks one behind the other without a flush (memLevel 1: a block every 127 symbols), so that headers and tables
    # begin at every bit of a byte -- the streams above have theirs on byte boundaries, behind a flush; starts: None, the
    # headers are found by asking the oracle where every prefix stands (cuts_of)
    d = make_block("alice", 5000, seed=29)
    co = zlib.compressobj(6, zlib.DEFLATED, -15, 1)
    out.append(Stream("small-blocks", d, co.compress(d) + co.flush(), None))
    return out


def _stored_starts(c):
    """the headers of a stream of stored blocks only"""
    starts, h = [], 0
    while h < len(c):
        starts.append(h)
        h += 5 + (c[h + 1] | c[h + 2] << 8)
    assert h == len(c) and c[starts[-1]] == 1
    return starts


def _scanned_cuts(s, rnd, body_samples):
    """cuts_of for a stream whose headers lie anywhere: of the cuts that stop in a header or table, the first and last three,
    every fourth between them and two on either side; and a sample of the cuts that stop in a body"""
    n = len(s.comp)
    inside, body = {}, []
    for k in range(1, n):
        _, st = O.inflate(s.comp[:k], CAP_MAX)
        if (st.out_sfbt & 0xe) == 0xe:
            inside.setdefault(8 * k - st.out_subc, []).append(k)
        else:
            body.append(k)
    ks = set()
    for v in inside.values():
        ks.update(v[:3] + v[3:-3:4] + v[-3:] + [v[0] - 2, v[0] - 1, v[-1] + 1, v[-1] + 2])
    ks.update(rnd.sample(body, body_samples * 3))
    return [(k, False) for k in sorted(ks) if 1 <= k < n]


def _state_of(st):
    kw = dict(subc=st.out_subc % 8, sfbt=st.out_sfbt, rembytecnt=st.out_rembytecnt if (st.out_sfbt & 0xe) == 0x8 else 0)
    if (st.out_sfbt & 0xe) == 0xc:
        kw.update(dht=bytes(st.out_dht), dhtlen=st.out_dhtlen)
    return kw


def header_end(s, h):
    """the byte behind the header of the block at h: behind LEN/NLEN, or the byte the table ends in (found with the oracle:
    the first cut behind which it no longer stands in the header)"""
    btype = (s.comp[h] >> 1) & 3
    if btype == 0:
        return h + 5
    if btype == 1:
        return h + 1
    for e in range(h + 3, min(len(s.comp), h + 330) + 1):
        _, st = O.inflate(s.comp[h:e], CAP_MAX)
        if st.err or (st.out_sfbt & 0xe) != 0xe:
            return e
    raise AssertionError("no end of the table at %d of %s" % (h, s.name))


def cuts_of(s, rnd, body_samples):
    """[(k, forced)]: the header bands, the edges of stored blocks and a seeded sample of every body; forced marks the
    body samples of dynamic blocks that are to resume with the whole rest behind an aligned start (the cut route's)"""
    if s.starts is None:
        return _scanned_cuts(s, rnd, body_samples)
    n = len(s.comp)
    ks = {}
    ends = s.starts[1:] + [n]
    for h, nxt in zip(s.starts, ends):
        e = header_end(s, h)
        # (the block in front ends with the empty stored block of a flush, whose header lies in the 5-6 bytes in front of h)
        for k in range(max(1, h - 7), min(n, e + 2) + 1):
            ks.setdefault(k, False)
        btype = (s.comp[h] >> 1) & 3
        if btype == 0:
            for k in (h + 6, nxt - 1, nxt - 2):
                if h + 5 < k < nxt:
                    ks.setdefault(k, False)
        lo, hi = e + 3, nxt - 1
        if hi > lo:
            for i in range(body_samples * (2 if btype else 1)):
                k = rnd.randrange(lo, hi)
                ks.setdefault(k, False)
                if btype == 2 and i % 2 == 0:
                    ks[k] = True
    return sorted(ks.items())


def _make(s, k, m_mode, layout_want, rnd, short, forced=False):
    c = s.comp + TRAILER
    out1, st1 = O.inflate(s.comp[:k], CAP_MAX)
    assert st1.err == 0 and not st1.final_eob
    back = (st1.out_subc + 7) // 8
    pos = k - back
    state = _state_of(st1)
    if m_mode == "rest":
        m = len(c) - pos
    elif m_mode == "cut":
        m = rnd.randrange(back + 1, max(back + 2, min(len(c) - pos, 6000)))
    else:
        m = int(m_mode)
    part2 = c[pos:pos + m]
    hist = out1[-32768:]
    layout, shift, pad = layout_want, 0, 0
    if layout == "b":
        pad = (-len(hist)) % 16
        if len(hist) + pad > 32768:
            layout = "a"
    if layout == "a":
        shift, pad = rnd.randrange(16), 0
    ohist = b"" if layout == "c" else bytes(pad) + hist
    exp, st = O.inflate(part2, CAP_MAX, hist=ohist, **state)
    cap = st.tpbc + rnd.choice([0, 16, 1000, 4096])
    if short and st.err == 0 and st.tpbc > 0:
        cap = st.tpbc - 1
    exp, st = O.inflate(part2, cap, hist=ohist, **state)
    return Case(stream=s.name, k=k, m=m, layout=layout, shift=shift, pad=pad, hist=b"" if layout == "c" else hist, part2=part2,
                subc1=st1.out_subc, subc=state["subc"], sfbt=state["sfbt"], rem=state["rembytecnt"], dht=state.get("dht", b""), dhtlen=state.get("dhtlen", 0),
                crc1=zlib.crc32(out1), adler1=zlib.adler32(out1), cap=cap, err=st.err, out=exp, tpbc=st.tpbc,
                out_sfbt=st.out_sfbt, out_subc=st.out_subc, out_rem=st.out_rembytecnt, out_dht=bytes(st.out_dht),
                out_dhtlen=st.out_dhtlen, final_eob=bool(st.final_eob), pos=pos, forced=forced)


def resume_word(c):
    return c.rem | c.sfbt << 16 | c.subc << 20


def build_cases(seed=7, body_samples=6):
    rnd = random.Random(seed)
    cases = []
    zero_done = set()
    for s in streams():
        for k, forced in cuts_of(s, rnd, body_samples):
            if forced:
                m_mode, layout = "rest", "b"
            else:
                m_mode = rnd.choice(["rest", "rest", "rest", "1", "2", "7", "cut", "cut"])
                layout = rnd.choice(["a", "a", "a", "a", "b", "b", "b", "c", "c"])
            short = not forced and rnd.randrange(10) == 0
            case = _make(s, k, m_mode, layout, rnd, short, forced)
            cases.append(case)
            kind = case.sfbt & 0xe
            if kind not in zero_done:                        # an empty part 2, once per kind
                zero_done.add(kind)
                cases.append(_make(s, k, "0", "a", rnd, False))
    return cases


_cached = None


def cases():
    """the set (built once a process)"""
    global _cached
    if _cached is None:
        _cached = build_cases()
    return _cached


def source_layout(c):
    """(bytes in front of the job's src inside a 16-byte aligned slot, the job's bytes [history][part 2], hist_len)"""
    if c.layout == "a":
        return c.shift, c.hist + c.part2, len(c.hist)
    if c.layout == "b":
        return 0, bytes(c.pad) + c.hist + c.part2, c.pad + len(c.hist)
    return 0, c.part2, 0


def oracle_hist(c):
    return bytes(c.pad) + c.hist


def oracle_state(c):
    kw = dict(subc=c.subc, sfbt=c.sfbt, rembytecnt=c.rem)
    if (c.sfbt & 0xe) == 0xc:
        kw.update(dht=c.dht, dhtlen=c.dhtlen)
    return kw
