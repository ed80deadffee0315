"""tests/inflate_part_model.py (the expected value of tests/test_gpu_inflate_part.py) against zlib.decompressobj fed the same parts
(wbits -15 / 15 / 31): the concatenated output is equal, unused_data matches in_used on DONE, eof matches -- for every stream of
resume_cases.streams() in all three framings and every cut family of the GPU suite: two parts at resume_cases' cuts and at every
byte of the framing, seeded splits into 3 to 9 parts with empty ones among them, 1-byte parts over the first 64 and the last 12
bytes, targets that fill.  And the tail's capacity: the longest dynamic header RFC 1951 allows, at each bit offset, cut one byte
before its end."""
import random
import struct
import zlib

import pytest

import deflate_handmade as H
import inflate_part_model as M
import oracle_lib as O
import resume_cases as R

WBITS = {M.FMT_RAW: -15, M.FMT_ZLIB: 15, M.FMT_GZIP: 31}
GZ_HEAD = b"\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\x03"


def framed(s, fmt):
    """(header, stream bytes) of a resume_cases stream in a framing"""
    if fmt == M.FMT_RAW:
        return b"", s.comp
    if fmt == M.FMT_ZLIB:
        return b"\x78\x9c", b"\x78\x9c" + s.comp + struct.pack(">I", zlib.adler32(s.data))
    return GZ_HEAD, GZ_HEAD + s.comp + struct.pack("<II", zlib.crc32(s.data), len(s.data))


def two_part_cuts(s, fmt, seed=5, body_samples=2):
    """resume_cases' cut set moved behind the header, and every byte of the framing"""
    head, z = framed(s, fmt)
    ks = {len(head) + k for k, _ in R.cuts_of(s, random.Random(seed), body_samples)}
    ks.update(range(1, len(head) + 1))
    ks.update(range(len(head) + len(s.comp), len(z)))
    return sorted(k for k in ks if 0 < k < len(z))


def many_part_splits(z, rnd):
    n = rnd.randrange(3, 10)
    at = sorted(rnd.choice([rnd.randrange(len(z) + 1), rnd.randrange(len(z) + 1), 0, len(z)]) if i % 3 == 0 else rnd.randrange(len(z) + 1)
                for i in range(n - 1))
    at = [0] + at + [len(z)]
    if n > 3:
        at[2] = at[1]                                                  # a part of length 0
        at.sort()
    return [z[a:b] for a, b in zip(at, at[1:])]


def byte_parts(z):
    a, b = min(64, len(z)), max(min(64, len(z)), len(z) - 12)
    return [z[i:i + 1] for i in range(a)] + [z[a:b]] + [z[i:i + 1] for i in range(b, len(z))]


def against_zlib(fmt, parts, data, extra=b""):
    calls, got = M.run(fmt, parts)
    d = zlib.decompressobj(WBITS[fmt])
    want = b"".join(d.decompress(p) for p in parts)
    assert got == want == data
    last = calls[-1][1]
    assert d.eof == (last["status"] == M.S_DONE)
    if d.eof:
        fed = sum(len(p) for p in parts[:len(calls)])
        assert len(d.unused_data) == len(b"".join(parts)) - (fed - len(parts[len(calls) - 1]) + last["in_used"])
    c = calls[-1][0]
    assert c["total_out"] == len(data) and c["crc"] == zlib.crc32(data) and c["adler"] == zlib.adler32(data)
    assert all(len(cc["tail"]) <= M.TAIL for cc, _, _ in calls)


STREAMS = R.streams()


@pytest.mark.parametrize("fmt", [M.FMT_RAW, M.FMT_ZLIB, M.FMT_GZIP])
@pytest.mark.parametrize("s", STREAMS, ids=[s.name for s in STREAMS])
def test_two_parts(s, fmt):
    _, z = framed(s, fmt)
    for k in two_part_cuts(s, fmt):
        against_zlib(fmt, [z[:k], z[k:] + b"beyond"], s.data)


@pytest.mark.parametrize("fmt", [M.FMT_RAW, M.FMT_ZLIB, M.FMT_GZIP])
@pytest.mark.parametrize("s", STREAMS, ids=[s.name for s in STREAMS])
def test_many_parts(s, fmt):
    _, z = framed(s, fmt)
    rnd = random.Random(11)
    for _ in range(6):
        against_zlib(fmt, many_part_splits(z, rnd), s.data)
    against_zlib(fmt, byte_parts(z), s.data)


@pytest.mark.parametrize("fmt", [M.FMT_RAW, M.FMT_ZLIB, M.FMT_GZIP])
@pytest.mark.parametrize("s", STREAMS, ids=[s.name for s in STREAMS])
def test_full_targets(s, fmt):
    head, z = framed(s, fmt)
    rnd = random.Random(13)
    for _ in range(4):
        k = rnd.randrange(len(head) + 1, len(z))
        caps = [rnd.randrange(1, min(3000, len(s.data) // 8)), rnd.randrange(300, 70000), 1 << 20]
        calls, got = M.run(fmt, [z[:k], z[k:]], caps, whole=s.comp)
        assert got == s.data and calls[-1][1]["status"] == M.S_DONE
        assert any(r["status"] == M.DST_FULL for _, r, _ in calls)
        for (c, r, out) in calls:
            assert len(c["tail"]) <= M.TAIL and r["out_len"] == len(out)
            if r["status"] == M.DST_FULL:
                assert r["cc"] == M.CC_DATA_LENGTH


def test_whole_stream_in_one_part_is_the_framed_answer():
    for s in STREAMS:
        for fmt in (M.FMT_ZLIB, M.FMT_GZIP):
            head, z = framed(s, fmt)
            c, r, out = M.part(None, fmt, z + b"xyz", 1 << 20, b"", M.FIRST)
            assert out == s.data and r["status"] == M.S_DONE and r["in_used"] == len(z) == c["frame"]["end"]
            assert c["frame"]["hdr_len"] == len(head) and c["frame"]["status"] == 0


def test_tail_capacity_is_the_longest_header():
    assert M.tail_capacity() == M.TAIL == 288
    text = open(__file__.replace("test_inflate_part_model_host.py", "../include/nxz_engine.h")).read()
    assert "#define NXZ_INFLATE_PART_TAIL 288" in text
    # every one of the 316 lengths coded singly with a 7-bit code: the lengths in use (4, 5, 8, 9) get the code-length code's longest codes
    cl = [1, 2, 3, 4, 7, 7, 5, 0, 7, 7] + [0] * 9
    assert H.kraft(cl) == 1.0
    for off in range(8):
        w = H.Bits()
        w.put(0, off)                                                  # (bits of the byte in front: in_subc = 8 - off)
        coder = H.dynamic(w, 1, H.GEN_LL, H.GEN_DD, hclen=19, cl=cl)
        nbits = w.n - off
        assert nbits == 3 + 14 + 19 * 3 + 316 * 7
        coder.eob()
        raw = w.data()
        out, st = O.inflate(raw, 1 << 16, subc=(8 - off) % 8)
        assert st.err == 0 and st.final_eob and out == b""             # the header is one the decoder takes
        cut = raw[:(off + nbits + 7) // 8 - 1]
        _, st = O.inflate(cut, 1 << 16, subc=(8 - off) % 8)
        assert st.err == 0 and (st.out_sfbt & 0xe) == 0xe and st.out_subc == 8 * len(cut) - off
        assert (st.out_subc + 7) // 8 <= M.TAIL
        c = M.start(M.FMT_RAW)
        c["subc"] = (8 - off) % 8
        c2, r, out = M.part(c, M.FMT_RAW, cut, 1 << 16)
        assert r["status"] == M.MORE and r["in_used"] == len(cut) and out == b""
        assert c2["tail"] == cut[len(cut) - (st.out_subc + 7) // 8:] and c2["sfbt"] & 0xe == 0xe and c2["subc"] == (8 - off) % 8
        # ... and the rest finishes the stream from the tail
        c3, r, out = M.part(c2, M.FMT_RAW, raw[len(cut):], 1 << 16)
        assert r["status"] == M.S_DONE and out == b""
    assert len(cut) == 286                                              # (off = 7: 2293 bits, 287 bytes, one short)
