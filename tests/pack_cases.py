"""Hand-made jobs and results for the member packers (tests/test_gpu_compress_edges.py part B; checked on the CPU by
tests/test_pack_model_host.py).  A case is the tuple tests/pack_model.py takes: (length, hist_len, cc, tpbc, crc, adler, src, dst).
src and dst hold seeded random bytes, so a copy from the wrong place shows; crc and adler are those of the source, so a stored
member is a stream zlib accepts.  dst of a case marked real (REAL_FROM on) holds a deflate block of the source."""
import functools
import zlib

import numpy as np

LENGTHS = (0, 1, 2, 3, 4, 5, 1000, 65279, 65280, 65535, 65536)
HISTORIES = (0, 16, 32768)
DICT = bytes(range(256)) * 9 + b"a preset dictionary"        # pack_zlib_dict only names it: DICTID = its Adler-32


def compress_bound(n):
    """nxz_compress_bound (power-gzip_amd/csrc/nxz_engine.cpp)"""
    return ((n * 9 + 7) // 8 + 16 + 15) & ~15


def pairs(length):
    """(cc, tpbc): compressed with 1 byte and just below the fallback threshold; at and past it; did not shrink (64); failed"""
    out = [(0, 1), (0, length + 4), (0, length + 5), (0, length + 6), (64, length + 9), (13, 0), (66, 0)]
    return [p for p in out if p[1] <= compress_bound(length)]


def _bytes(seed, n):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def _case(seed, length, hist, cc, tpbc):
    src = _bytes(2 * seed, hist + length)
    dst = _bytes(2 * seed + 1, max(tpbc, 1))
    source = src[hist:]
    return (length, hist, cc, tpbc, zlib.crc32(source), zlib.adler32(source), src, dst)


def _real(seed, length):
    """a source that shrinks and its raw deflate block as dst: what a compress job leaves behind"""
    source = (b"%d bottles of beer on the wall, " % seed) * (length // 24 + 1)
    source = source[:length]
    co = zlib.compressobj(6, zlib.DEFLATED, -15)
    dst = co.compress(source) + co.flush()
    assert len(dst) < length + 5
    return (length, 0, 0, len(dst), zlib.crc32(source), zlib.adler32(source), source, dst)


@functools.lru_cache(maxsize=None)
def table():
    """every length x history x (cc, tpbc) with length + history <= 65536, then a few real deflate blocks.  Jobs that differ in
    one step of length or tpbc follow each other, so the members' starts run through the residues mod 4."""
    out, seed = [], 0
    for length in LENGTHS:
        for hist in HISTORIES:
            if length + hist > 65536:
                continue
            for cc, tpbc in pairs(length):
                seed += 1
                out.append(_case(seed, length, hist, cc, tpbc))
    real_from = len(out)
    out += [_real(i, n) for i, n in enumerate((64, 1000, 1001, 1002, 1003, 65535, 65536))]
    return tuple(out), real_from


def many(n):
    """n tiny jobs (length <= 64) for the launches that give a thread of the offsets kernel more than one job"""
    small = (0, 1, 2, 3, 4, 5, 17, 64)
    out = []
    for i in range(n):
        length = small[(i * 5 + i // 8) % len(small)]
        cc, tpbc = pairs(length)[(i * 3 + i // 7) % 7]
        out.append(_case(100000 + i, length, 16 * (i % 3 == 1), cc, tpbc))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def launches():
    """name -> cases: the table; n = 1, 1023, 1024, 1025 and 2050.  The offsets kernel has 1024 threads with per = ceil(n / 1024)
    jobs each: 1025 gives two a thread, thread 512 one and the threads behind it none; 2050 three a thread, thread 683 one."""
    t, _ = table()
    big = many(2050)
    return {"table": t, "1": (t[40],), "1023": big[:1023], "1024": big[:1024], "1025": big[:1025], "2050": big}
