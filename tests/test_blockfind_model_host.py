"""tests/blockfind_model.py held to zlib and to the oracle, and tests/blockfind_cases.py held to the conditions under which
the comparison with the kernels is exact.  No GPU.

  every true start of a dynamic block in streams zlib writes (levels 1, 6, 9, Z_FILTERED; the boundaries from zlib's own
  inflate with Z_BLOCK: tests/checkpoint_model.py) and in a block with the table generator's table (286 / 30 / 19: the
  oracle's dhtgen) passes the rule;
  every hand-built header that must pass passes, and every one that must not fails for the reason it is named after;
  every segment of every built case is one the model can speak for: K <= 1024, and either K <= 126 (the second kernel does
  the segment) or more than 126 passers (the first kernel does it itself)."""
import ctypes as C
import zlib

import numpy as np
import pytest

import blockfind_cases as Cs
import blockfind_model as M
import checkpoint_model as CM
import deflate_handmade as H
import oracle_lib as O


def _text(n):
    rng = np.random.default_rng(11)
    words = [bytes(rng.integers(97, 123, int(k), dtype=np.uint8)) for k in rng.integers(2, 9, 400)]
    return b" ".join(words[int(i)] for i in rng.integers(0, 400, n // 5))[:n]


@pytest.mark.parametrize("level,strategy", [(1, zlib.Z_DEFAULT_STRATEGY), (6, zlib.Z_DEFAULT_STRATEGY), (9, zlib.Z_DEFAULT_STRATEGY),
                                            (6, zlib.Z_FILTERED)])
def test_every_dynamic_block_zlib_writes_passes(level, strategy):
    data = _text(300000)
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 6, strategy)           # (memLevel 6: blocks of 8 Ki symbols, a dozen of them)
    comp = c.compress(data) + c.flush()
    headers, end, plain = CM.block_boundaries(comp, CM.FMT_RAW)
    assert end is not None and plain == data
    bits = M.bits_of(comp)
    dyn = [b for b, _ in headers if bits[b + 1] == 0 and bits[b + 2] == 1]
    assert len(dyn) >= 4
    for b in dyn:
        v = M.header(bits, b, 8 * len(comp))
        assert v.ok, (b, v)


def test_the_table_generators_header_passes():
    ll = (C.c_uint32 * 286)(*([1] * 286))
    dd = (C.c_uint32 * 30)(*([1] * 30))
    for k, b in enumerate(b"a table of the generator"):
        ll[b] += 50 + k
    dht, dhtlen = O.dhtgen(ll, dd)
    w = H.Bits()
    w.put(0, 1); w.put(2, 2)
    w.bits(bytes(dht), dhtlen)
    bits = M.bits_of(w.data())
    assert (sum(bits[3 + k] << k for k in range(5)), sum(bits[8 + k] << k for k in range(5)), sum(bits[13 + k] << k for k in range(4))) == (29, 29, 15)
    v = M.header(bits, 0, w.n)
    assert v.ok and v.end == w.n, v


@pytest.mark.parametrize("name", Cs.MUST_PASS)
def test_headers_that_must_pass(name):
    data, n, _ = Cs.HEADERS[name]
    v = M.header(M.bits_of(data), 0, n)
    assert v.ok and v.end == n, v
    assert not M.header(M.bits_of(data), 0, n - 1).ok            # (and not with its last bit behind the limit)
    # zlib takes the header as well: a block of end-of-block only behind it ends the stream (or, with no code it could use
    # wrongly, zlib fails behind the header and not in it)
    assert "invalid code lengths" not in _zlib_says(data, n) and "invalid bit length" not in _zlib_says(data, n)


def _zlib_says(data, n):
    buf = bytearray(data) + bytes(64)
    buf[0] |= 1
    try:
        zlib.decompressobj(-15).decompress(bytes(buf))
    except zlib.error as e:
        return str(e)
    return ""


@pytest.mark.parametrize("name", Cs.MUST_NOT)
def test_headers_that_must_not_pass(name):
    data, n, reason = Cs.HEADERS[name]
    v = M.header(M.bits_of(data + bytes(64)), 0, 8 * (len(data) + 64))
    assert not v.ok and v.reason == reason, v


def test_the_smallest_header_and_the_longest():
    assert Cs.HEADERS["the-smallest-hclen-5-hlit-257-hdist-1"][0][:2] == bytes([0x04, 0x20])      # BTYPE 10, HLIT 0, HDIST 0, HCLEN 1 (bit 13)
    assert Cs.HEADERS[Cs.LONGEST][1] == 17 + 19 * 3 + 316 * 7 and (Cs.HEADERS[Cs.LONGEST][1] + 7) // 8 + 1 <= M.LOOK


@pytest.mark.parametrize("S", Cs.SEGS)
def test_every_segment_of_every_case_is_one_the_model_speaks_for(S):
    seen = set()
    for c in Cs.built(S):
        for T in (S,):
            e = Cs.expected(c, T)
            assert max(e.K) <= M.MAXCAND, (c.name, e.K)
            for g in range(e.nseg):
                cls = M.segment_class(e.K[g], e.npass[g])
                assert cls is not None, (c.name, g, e.K[g], e.npass[g])
                seen.add(cls)
                first, more = e.first[g], [x for x in e.more[g] if x != M.NONE]
                assert (first == M.NONE) == (e.npass[g] == 0) and len(more) == min(3, max(0, e.npass[g] - 1))
                assert more == sorted(more, reverse=True) and all(x > first for x in more)
        # what a case is named after is there: its headers that pass alone and lie whole inside the stream are passers
        for bit, h in c.placed:
            n = Cs.HEADERS[h][1]
            if Cs.HEADERS[h][2] == "ok" and bit + n <= 8 * len(c.src) and not any(bit < b2 < bit + n for b2, _ in c.placed):
                assert Cs.scan(c).passes(bit, 8 * len(c.src)), (c.name, bit, h)
    assert seen == ({"two", "one"} if S >= 2048 else {"two"})


def test_segment_sizes_restated():
    assert [M.segment_bytes(n) for n in (1 << 20, (1 << 20) + 1, 2 << 20, (2 << 20) + 1, 8 << 20, (8 << 20) + 1)] == [1024, 2048, 2048, 4096, 4096, 8192]
