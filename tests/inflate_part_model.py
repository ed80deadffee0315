"""nxz_batch_inflate_streams_part (include/nxz_engine.h: a stream read in parts) as a Python model over the CPU oracle -- no engine
import.  A part's decode is oracle_lib.inflate(src, cap, hist, **resume) with the state built as resume_cases._state_of does;
headers and trailers are tests/framing.py's; the tail, in_used and status rules are written out here.  The oracle has no
"suspend when full": where a full target suspends comes from the token walker of tests/checkpoint_fine_model.py on the whole
deflate data (the stream stands in front of the first byte-making token that does not fit; a stored block splits at the byte).

part() takes the carry (a dict, or None with FIRST) and returns (carry, result, output bytes); it is the expected value of
tests/test_gpu_inflate_part.py and is itself held to zlib.decompressobj in tests/test_inflate_part_model_host.py."""
import zlib

import checkpoint_fine_model as W
import framing as F
import oracle_lib as O
from resume_cases import _state_of

TAIL = 288
WINDOW = 32768
FMT_RAW, FMT_ZLIB, FMT_GZIP, FMT_AUTO = 0, 1, 2, 3
FIRST = 1
HEADER, BODY, TRAILER, DONE, FAILED = range(5)                       # phase
MORE, S_DONE, DST_FULL, S_FAILED = range(4)                           # status
CC_OK, CC_DATA_LENGTH, CC_INVALID_OP, CC_TARGET_SPACE = 0, 3, 8, 13
FRAME_FIELDS = F.FIELDS + ("end", "check", "isize")


def tail_capacity():
    """RFC 1951: BFINAL / BTYPE, HLIT HDIST HCLEN, 19 code length code lengths, 316 lengths coded singly with 7-bit codes, started
    at the last bit of a byte; in bytes, rounded up to a multiple of 16"""
    bits = 3 + 14 + 19 * 3 + 316 * 7 + 7
    return ((bits + 7) // 8 + 15) & ~15


def refusal(src_len, dst_cap, prev_len, flags, phase, src_null=False, dst_null=False, prev_null=False):
    if (src_null and src_len) or (dst_null and dst_cap) or (prev_null and prev_len) or flags & ~FIRST or (flags & FIRST and prev_len):
        return CC_INVALID_OP
    if not flags & FIRST and phase >= DONE:
        return CC_INVALID_OP
    return 0


def start(fmt):
    frame = dict.fromkeys(FRAME_FIELDS, 0)
    frame["format"] = FMT_GZIP if fmt == FMT_GZIP else FMT_RAW if fmt == FMT_RAW else FMT_ZLIB
    return dict(phase=BODY if fmt == FMT_RAW else HEADER, frame=frame, header=b"", sfbt=0, rem=0, dhtlen=0, dht=b"", subc=0, crc=0, adler=1,
                parts=0, tail=b"", total_in=0, total_out=0)


def _result(c, cc, status, in_used, out_len):
    return dict(cc=cc, status=status, in_used=in_used, out_len=out_len, crc=c["crc"], adler=c["adler"])


def _trailer_len(fmt):
    return {FMT_RAW: 0, FMT_ZLIB: 4, FMT_GZIP: 8}[fmt]


def _trailer_take(c, b):
    k = min(len(b), _trailer_len(c["frame"]["format"]) - len(c["tail"]))
    c["tail"] += b[:k]
    return k


def _trailer_finish(c):
    f = c["frame"]
    tl = _trailer_len(f["format"])
    if len(c["tail"]) != tl:
        return False
    st = F.OK
    if tl:
        # framing.trailer on a source that is the trailer alone: the decoder took nothing of it and left nothing
        res = dict(cc=CC_OK, sfbt=F.SFBT_FINAL_EOB, spbc=0, subc=0, tpbc=c["total_out"] & 0xffffffff, crc=c["crc"], adler=c["adler"])
        st, _, f["check"], f["isize"] = F.trailer(c["tail"], f["format"], 0, res)
    f["status"], f["end"] = st, c["total_in"] & 0xffffffff
    c["tail"] = b""
    c["phase"] = DONE if st == F.OK else FAILED
    return True


def _full_stop(whole, bit0, u0, cap):
    """where a decode that stands at bit `bit0` of the deflate data `whole` with u0 bytes of output suspends on a target of cap
    bytes: (bit, sfbt, rem, tbit, dhtlen) of the first byte-making token at or behind bit0 that does not fit"""
    tokens, _, _ = W.walk_cached(whole, W.FMT_RAW)
    stop = u0 + cap
    for bit, u, n, count, sfbt, tbit, dhtlen, rem in tokens:
        if count == 1:
            if bit >= bit0 and u + n > stop:
                return bit, sfbt, 0, tbit, dhtlen
        elif u + count > stop and bit + 8 * (count - 1) >= bit0:
            i = max(stop - u, 0)
            return bit + 8 * i, sfbt, rem - i, 0, 0
    raise AssertionError("nothing fails to fit")


def part(c, fmt, src, cap, prev=b"", flags=0, whole=None, hdr_len=None):
    """one part of one stream.  c: the carry from the part before (not changed; None with FIRST); prev: the output bytes in front of
    the target; whole: the stream's raw deflate data, needed only where a target fills.  -> (carry, result, out)"""
    cc = refusal(len(src), cap, len(prev), flags, DONE if c is None and not flags & FIRST else c["phase"] if c else 0)
    if cc:
        return c, dict(cc=cc, status=S_FAILED, in_used=0, out_len=0, crc=0, adler=0), b""
    c = start(fmt) if flags & FIRST else dict(c, frame=dict(c["frame"]))
    body = 0
    while c["phase"] == HEADER and body < len(src):
        c["header"] += src[body:body + 1]
        body += 1
        f = F.parse(c["header"], fmt)
        if f["status"] == F.TRUNCATED:
            continue
        c["frame"].update(f)
        c["phase"] = BODY if f["status"] == F.OK else FAILED
    if not (c["phase"] == BODY and body < len(src)):
        status, used = MORE, len(src)
        if c["phase"] == TRAILER:
            used = _trailer_take(c, src)
            c["total_in"] += used
            if _trailer_finish(c):
                status = S_DONE if c["phase"] == DONE else S_FAILED
        elif c["phase"] == FAILED:
            status, used = S_FAILED, 0
        else:
            c["total_in"] += used
        c["parts"] += 1
        return c, _result(c, CC_OK, status, used, 0), b""
    # the decode of [tail][part from body] behind the window
    w = min(WINDOW, len(prev), c["total_out"])
    hist = prev[len(prev) - w:]
    told = len(c["tail"])
    s = c["tail"] + src[body:]
    L = len(s)
    state = dict(subc=c["subc"], sfbt=c["sfbt"], rembytecnt=c["rem"])
    if c["sfbt"] & 0xe == 0xc:
        state.update(dht=c["dht"], dhtlen=c["dhtlen"])
    out, st = O.inflate(s, cap, hist=hist, **state)
    c["parts"] += 1
    if st.err == CC_TARGET_SPACE:
        dpos = c["total_in"] + body - c["frame"]["hdr_len"] - told            # the byte of the deflate data s begins at
        if hdr_len is not None:
            assert hdr_len == c["frame"]["hdr_len"]
        bit, sfbt, rem, tbit, dhtlen = _full_stop(whole, 8 * dpos + (8 - c["subc"]) % 8, c["total_out"], cap)
        rel = bit - 8 * dpos
        cons = (rel + 7) // 8
        subc = cons * 8 - rel
        if sfbt & 0xe == 0x8:                                          # what fits of the stored block
            out, st2 = O.inflate(s[:cons], cap, hist=hist, **state)
            assert st2.err == 0 and len(out) == cap
        P = cons - (1 if subc else 0)
        dht = W.table_bits(whole, tbit, dhtlen) if sfbt & 0xe == 0xc else b""
        c.update(sfbt=sfbt, rem=rem, subc=subc, dhtlen=dhtlen, dht=dht)
        if cons == L:
            status, used, keep_to = MORE, len(src), L
        else:
            status, used, keep_to = DST_FULL, body + max(P - told, 0), max(P, told)
        c["tail"] = s[P:keep_to]
        cc = CC_DATA_LENGTH
    elif st.err:
        c["frame"]["status"] = F.DEFLATE
        c["phase"] = FAILED
        return c, _result(c, st.err, S_FAILED, 0, 0), b""
    elif st.final_eob:
        dend = L - st.out_subc // 8
        c["crc"], c["adler"] = zlib.crc32(out, c["crc"]), zlib.adler32(out, c["adler"])
        c["total_out"] += len(out)
        c.update(sfbt=0, rem=0, subc=0, dhtlen=0, dht=b"", tail=b"", phase=TRAILER)
        at = dend + _trailer_take(c, s[dend:])
        used = body + max(at - told, 0)
        c["total_in"] += used
        done = _trailer_finish(c)
        status = MORE if not done else S_DONE if c["phase"] == DONE else S_FAILED
        return c, _result(c, CC_OK if st.out_subc < 8 else CC_DATA_LENGTH, status, used, len(out)), out
    else:
        back = (st.out_subc + 7) // 8
        assert back <= TAIL and back <= L
        kw = _state_of(st)
        c.update(sfbt=kw["sfbt"], rem=kw["rembytecnt"], subc=kw["subc"], dhtlen=kw.get("dhtlen", 0),
                 dht=kw.get("dht", b"")[:(kw.get("dhtlen", 0) + 7) // 8])
        status, used, cc = MORE, len(src), CC_DATA_LENGTH
        c["tail"] = s[L - back:]
    c["crc"], c["adler"] = zlib.crc32(out, c["crc"]), zlib.adler32(out, c["adler"])
    c["total_out"] += len(out)
    c["total_in"] += used
    return c, _result(c, cc, status, used, len(out)), out


def run(fmt, parts, caps=None, whole=None):
    """a stream handed over as `parts` (bytes each), the outputs laid end to end, a target that fills sent again from in_used with a
    fresh one of the same cap -> [(carry, result, out)] per call, the concatenated output"""
    c, calls, data = None, [], b""
    for k, p in enumerate(parts):
        flags = FIRST if k == 0 else 0
        while True:
            cap = caps[len(calls) % len(caps)] if caps else 1 << 20
            c, r, out = part(c, fmt, p, cap, data[-WINDOW:] if not flags else b"", flags, whole)
            calls.append((c, r, out))
            data += out
            if r["status"] != DST_FULL:
                break
            p, flags = p[r["in_used"]:], 0
        if r["status"] in (S_DONE, S_FAILED):
            break
    return calls, data
