"""The model of the member packers (tests/pack_model.py) against zlib and gzip, on the case table the GPU test packs
(tests/pack_cases.py).  No GPU: what is checked here is that the model's members are what the header promises -- streams any
reader accepts --, so that the GPU test may take the model's bytes for the truth."""
import gzip
import zlib

import framing as F
import pack_cases as PC
import pack_model as M

LEVELS = (-1, 0, 1, 5, 9)
DICTID = zlib.adler32(PC.DICT)


def decodable(i, case, real_from):
    """a stored fallback, or a case whose dst holds a real deflate block (the others carry random bytes as payload)"""
    return M.is_stored(case[0], case[2], case[3]) or i >= real_from


def test_table_has_the_cases():
    cases, real_from = PC.table()
    seen = {(c[0], c[1]) for c in cases[:real_from]}
    assert seen == {(n, h) for n in PC.LENGTHS for h in PC.HISTORIES if n + h <= 65536}
    for n, h in seen:
        got = [(c[2], c[3]) for c in cases[:real_from] if (c[0], c[1]) == (n, h)]
        assert got == [(0, 1), (0, n + 4), (0, n + 5), (0, n + 6), (64, n + 9), (13, 0), (66, 0)], (n, h)
    assert all(c[3] <= PC.compress_bound(c[0]) for c in cases)
    # the threshold: tpbc = length + 4 is kept, length + 5 is stored
    assert not M.is_stored(1000, 0, 1004) and M.is_stored(1000, 0, 1005)


def test_members_start_at_every_residue():
    """stored and compressed members at packed + off = 0, 1, 2, 3 mod 4, for each packer, with `packed` itself aligned"""
    cases, _ = PC.table()
    for name in M.PACKERS:
        offs, _ = M.image(name, cases, dictid=DICTID)
        for stored in (False, True):
            res = {offs[i] % 4 for i, c in enumerate(cases) if M.is_stored(c[0], c[2], c[3]) == stored}
            assert res == {0, 1, 2, 3}, (name, stored, res)


def test_gzip_members_decode():
    cases, real_from = PC.table()
    for i, c in enumerate(cases):
        m = M.gzip_member(*c)
        assert len(m) == M.GZIP_OVERHEAD + M.payload_size(c[0], c[2], c[3])
        if len(m) <= 65536:
            assert F.bgzf_member_size(m + b"tail") == len(m), i
        else:
            assert m[16] | m[17] << 8 == (len(m) - 1) & 0xffff
        if decodable(i, c, real_from):
            assert gzip.decompress(m) == c[6][c[1]:], i


def test_zlib_members_decode():
    cases, real_from = PC.table()
    for level in LEVELS:
        ref = zlib.compressobj(level).compress(b"")[:2] if level else b"\x78\x01"
        for i, c in enumerate(cases):
            m = M.zlib_member(*c, level=level)
            assert m[:2] == ref and len(m) == M.ZLIB_OVERHEAD + M.payload_size(c[0], c[2], c[3])
            if decodable(i, c, real_from):
                assert zlib.decompress(m) == c[6][c[1]:], (level, i)


def test_zlib_dict_members_decode():
    cases, real_from = PC.table()
    for level in LEVELS:
        for i, c in enumerate(cases):
            m = M.zlib_dict_member(*c, level=level, dictid=DICTID)
            assert len(m) == M.ZLIB_DICT_OVERHEAD + M.payload_size(c[0], c[2], c[3])
            assert m[1] & 0x20 and (m[0] << 8 | m[1]) % 31 == 0 and m[1] >> 6 == M.zlib_cmf_flg(level, False)[1] >> 6
            if decodable(i, c, real_from):
                d = zlib.decompressobj(zdict=PC.DICT)
                assert d.decompress(m) == c[6][c[1]:] and d.eof and not d.unused_data, (level, i)


def test_a_source_of_65536_bytes_is_two_stored_blocks():
    c = [x for x in PC.table()[0] if x[0] == 65536 and x[2] == 13][0]
    p = M.payload(*c[:4], c[6], c[7])
    assert p[:5] == b"\x00\xff\xff\x00\x00" and p[5 + 65535:5 + 65535 + 5] == b"\x01\x01\x00\xfe\xff" and len(p) == 65536 + 10
    d = zlib.decompressobj(-15)
    assert d.decompress(p) == c[6] and d.eof


def test_totals_stay_within_the_documented_bound():
    for name, cases in PC.launches().items():
        for packer in M.PACKERS:
            offs, img = M.image(packer, cases, dictid=DICTID)
            assert offs[-1] == len(img) <= M.packed_bound(packer, cases), (name, packer)
            assert offs == sorted(offs) and len(offs) == len(cases) + 1
    assert [len(v) for v in PC.launches().values()] == [len(PC.table()[0]), 1, 1023, 1024, 1025, 2050]
    assert all(c[0] <= 64 for c in PC.launches()["2050"])
