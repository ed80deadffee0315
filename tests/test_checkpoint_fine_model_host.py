"""The model of the fine checkpoint index (tests/checkpoint_fine_model.py: a token walker and the budget rule in Python) proven on
the CPU before the GPU is held to it.  Its block headers and out_len are those of system zlib's inflate(Z_BLOCK)
(checkpoint_model.block_boundaries) on every test stream; and every segment of every fine index, decoded by the oracle's
resumable decoder from the segment's source bytes alone -- the window as history, the state entry as resume fields, the table bits
cut out of the source --, gives back exactly the plain bytes of the segment."""
import pytest

import checkpoint_fine_model as F
import checkpoint_model as M
import oracle_lib

SPANS = [258, 1000, 4096, 65536]
STREAMS = F.streams()
IDS = [s[0] for s in STREAMS]


@pytest.mark.parametrize("name,fmt,stream,plain", STREAMS, ids=IDS)
def test_block_headers_are_zlibs(name, fmt, stream, plain):
    headers, end, zplain = M.block_boundaries(stream, fmt)
    w = F.walk_cached(stream, fmt)
    if plain is None:
        assert w is None and end is None
        return
    tokens, fheaders, fend = w
    assert zplain == plain and fheaders == headers and fend == end and end[1] == len(plain)
    # the tokens make the output, in order, without gaps
    u = 0
    for bit, tu, n, count, sfbt, tbit, dhtlen, rem in tokens:
        assert tu == u and n >= 1 and count >= 1 and (count == 1 or (n == 1 and sfbt & 0xe == 0x8 and rem == count and bit % 8 == 0))
        u += n * count
    assert u == len(plain)


def test_the_stream_set_covers_the_branches():
    by = {s[0]: s for s in STREAMS}
    kinds = lambda name: {t[4] & 0xe for t in F.walk_cached(by[name][2], by[name][1])[0]}
    assert kinds("fixed_one_block") == {0xa} and len(F.walk_cached(by["fixed_one_block"][2], F.FMT_RAW)[1]) == 1
    assert kinds("stored") == {0x8} and kinds("alice6_raw") == {0xc}
    assert all(t[2] == 258 for t in F.walk_cached(by["rle_zeros"][2], F.FMT_ZLIB)[0][1:-1])          # a literal, then nothing but 258-byte matches (the last one shorter)
    tokens, headers, end = F.walk_cached(by["empty_final_block"][2], F.FMT_RAW)
    assert headers[-1][1] == end[1] == 110000                                                    # the final block makes nothing
    assert len(F.walk_cached(by["mem1"][2], F.FMT_GZIP)[1]) > 100 and by["alice6_gzip_fields"][2][3] == 0x1e


@pytest.mark.parametrize("span", SPANS + [1 << 20])
@pytest.mark.parametrize("name,fmt,stream,plain", [s for s in STREAMS if s[3] is not None], ids=[s[0] for s in STREAMS if s[3] is not None])
def test_every_segment_decodes_to_the_plain_bytes(name, fmt, stream, plain, span):
    idx = F.index(stream, fmt, span)
    n = idx["count"]
    assert idx["out_len"] == len(plain) and idx["uoff"][0] == 0 and idx["state"][0] == (0, 0, 0) and idx["state"][n] == (0, 0, 0)
    assert idx["cbit"][0] == 8 * F.header_len(stream, fmt)
    sizes = [idx["uoff"][k + 1] - idx["uoff"][k] for k in range(n)]
    assert all(span - 257 <= s <= span for s in sizes[:-1]) and sizes[-1] <= span
    assert all(a < b for a, b in zip(idx["cbit"], idx["cbit"][1:])) and all(a < b for a, b in zip(idx["uoff"][:n], idx["uoff"][1:n]))
    if span > len(plain):
        assert n == 1
    if name == "rle_zeros" and span == 1000:
        assert all(s == 774 for s in sizes[1:-1]) and sizes[0] == 775                           # 3 x 258 (the first: a literal in front)
    if name == "stored":
        assert all(s == span for s in sizes[:-1])                                                # a stored run splits at exactly span bytes
    if name == "fixed_one_block":
        assert n > 1 or span >= len(plain)                                                       # the case the coarse index cannot cut
    for k in range(n):                                                                           # every segment through the oracle
        b, e, in_subc, wlen, olen, sfbt, rem, tbit, dhtlen = F.segment(idx, k)
        u0 = idx["uoff"][k]
        resume = dict(subc=in_subc, sfbt=sfbt, rembytecnt=rem)
        if sfbt & 0xe == 0xc:
            resume.update(dht=F.table_bits(stream, tbit, dhtlen), dhtlen=dhtlen)
        out, st = oracle_lib.inflate(stream[b:e], cap=olen, hist=plain[u0 - wlen:u0], **resume)
        # err 0: the stream's end, or suspended where the source ran out; 13: a short token whole inside the bits behind the boundary
        assert st.err in (0, 13), (k, st.err)
        assert out[:olen] == plain[u0:u0 + olen] and (st.err == 13 or st.tpbc == olen), (k, st.err, st.tpbc, olen)
