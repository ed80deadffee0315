"""The model of the checkpoint index (tests/checkpoint_model.py: block headers from system zlib's inflate(Z_BLOCK), the checkpoint
rule in Python) proven on the CPU before the GPU is held to it: every segment of an index, decoded by zlib alone from the
segment's source bytes -- inflatePrime for the bits of the first byte, inflateSetDictionary for the window --, gives back exactly
the plain bytes of the segment."""
import zlib

import pytest

import checkpoint_model as M
import datagen

PLAIN = datagen.ALICE_LIKE(200000)


@pytest.mark.parametrize("level,mem_level,blocks,inside", [(6, 1, 292, 250), (1, 1, 451, 403), (6, 8, 3, None)])
def test_zlib_reports_the_block_headers(level, mem_level, blocks, inside):
    s = M.deflate(PLAIN, M.FMT_ZLIB, level, mem_level)
    headers, end, plain = M.block_boundaries(s, M.FMT_ZLIB)
    assert plain == PLAIN and end is not None and end[1] == len(PLAIN) and (end[0] + 7) // 8 == len(s) - 4
    assert headers[0] == (16, 0)
    assert all(a[0] < b[0] and a[1] <= b[1] for a, b in zip(headers, headers[1:]))
    # (the counts depend on zlib's block splitting: the ones of zlib 1.2.x / 1.3.x; the properties above hold for any)
    if zlib.ZLIB_RUNTIME_VERSION.startswith(("1.2.", "1.3")):
        assert len(headers) == blocks and (inside is None or sum(1 for b, _ in headers if b & 7) == inside)


@pytest.mark.parametrize("fmt", [M.FMT_RAW, M.FMT_ZLIB, M.FMT_GZIP])
@pytest.mark.parametrize("level,mem_level,strategy", [(6, 1, zlib.Z_DEFAULT_STRATEGY), (1, 1, zlib.Z_DEFAULT_STRATEGY), (6, 8, zlib.Z_DEFAULT_STRATEGY),
                                                      (0, 1, zlib.Z_DEFAULT_STRATEGY), (6, 1, zlib.Z_FIXED)])
@pytest.mark.parametrize("span", [1, 16384])
def test_every_segment_resumes_to_the_plain_bytes(fmt, level, mem_level, strategy, span):
    s = M.deflate(PLAIN, fmt, level, mem_level, strategy)
    idx = M.index(s, fmt, span)
    assert idx is not None and idx["out_len"] == len(PLAIN) and idx["uoff"][0] == 0
    assert idx["cbit"][0] == 8 * {M.FMT_RAW: 0, M.FMT_ZLIB: 2, M.FMT_GZIP: 10}[fmt]
    n = idx["count"]
    assert all(idx["uoff"][k + 1] - idx["uoff"][k] >= span for k in range(n - 1))
    if span == 16384 and mem_level == 1 and level:
        assert 8 <= n <= 16                                           # about a dozen
    assert any(c & 7 for c in idx["cbit"][:n]) or level == 0          # (stored blocks start where a byte does, after their header's padding)
    for k in range(n):
        assert M.resume(s, idx, k) == PLAIN[idx["uoff"][k]:idx["uoff"][k + 1]], k


def test_streams_that_fail_have_no_index():
    s = M.deflate(PLAIN, M.FMT_ZLIB, 6, 1)
    assert M.index(s[:len(s) // 2], M.FMT_ZLIB, 1) is None
    assert M.index(b"", M.FMT_RAW, 1) is None
    e = M.index(M.deflate(b"", M.FMT_GZIP), M.FMT_GZIP, 1)
    assert e["count"] == 1 and e["uoff"] == [0, 0] and e["cbit"][0] == 80 and M.resume(M.deflate(b"", M.FMT_GZIP), e, 0) == b""
