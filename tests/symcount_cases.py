"""Blocks for the symbol-count tests (tests/test_gpu_symbol_counts.py; checked on the CPU by tests/test_symcount_host.py).
A case is (name, data, hist_len): data[:hist_len] is history, the rest the block, at most 65536 bytes together.  The truth is
always the oracle's: counts(data, hist_len)."""
import functools
import random

import numpy as np

import oracle_lib as O
from datagen import make_block

LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193,
             12289, 16385, 24577)
# round the lane's 8 positions, the bitmap word, the round of 2048, the LZ77 tile and the block
LENGTHS = (0, 1, 2, 3, 7, 8, 9, 31, 32, 33, 2047, 2048, 2049, 16383, 16384, 16385, 65535, 65536)
# The batched interface takes histories that are a multiple of 16 (include/nxz_engine.h).  Histories of 1, 15 and 32767 bytes
# are given as a shared dictionary of that length, whose last W = min(len, 32768) & ~15 bytes reach the kernels as the window.
HISTORIES = (16, 4080, 32752, 32768)
DICT_HISTORIES = (1, 15, 32767)


def counts(data, hist=0):
    """the oracle's 316 counts of the block data[hist:] behind the history data[:hist], EOB counted once"""
    ll, d = O.counts(*O.lz77(data, hist))
    c = np.array(list(ll) + list(d), np.uint32)
    c[256] = 1
    return c


@functools.lru_cache(maxsize=None)
def every_symbol_block():
    """random bytes (literals of every value); copies of every length symbol's first and last length from 300..2000 back; copies
    of 40 bytes from every distance symbol's first and last distance back; runs of period 1..4 (length 258, the shortest
    distances); a match that the block's end cuts to 3 bytes.  Everything fenced by two fresh bytes.  That the oracle's parse
    uses all 29 + 30 symbols is tests/test_symcount_host.py's to check."""
    rnd = random.Random("symcount/every-symbol")
    buf = bytearray(rnd.randbytes(33500))
    for s, length in enumerate(LEN_BASE):
        for n in {length, LEN_BASE[s + 1] - 1 if s < 28 else 258}:
            at = len(buf) - rnd.randrange(300, 2000)
            buf += buf[at:at + n]
            buf += rnd.randbytes(2)
    for s, dist in enumerate(DIST_BASE):
        for back in {dist, DIST_BASE[s + 1] - 1 if s < 29 else 32768}:
            for _ in range(40):
                buf.append(buf[-back])
            buf += rnd.randbytes(2)
    for period in (1, 2, 3, 4):
        buf += rnd.randbytes(period) * (600 // period)
        buf += rnd.randbytes(2)
    at = len(buf) - 1000
    buf += buf[at:at + 3]
    return bytes(buf)


def text33(n, index=0):
    """bench.gen_text's 33-symbol text, block `index`, on the CPU"""
    import torch

    import bench
    return bench.gen_text(torch, torch.device("cpu"), 1, index, length=max(n, 1))[0].numpy().tobytes()[:n]


@functools.lru_cache(maxsize=None)
def small_batch():
    """about 40 jobs: every length in a content that suits it, the five contents at full size, every history"""
    kinds = ("zeros", "random", "text33", "ff")

    def content(kind, n, seed):
        if kind == "ff":
            return b"\xff" * n
        if kind == "text33":
            return text33(n, seed)
        return make_block(kind, n, seed=seed)
    out = [("%s/%d" % (kinds[i % 4], n), content(kinds[i % 4], n, i), 0) for i, n in enumerate(LENGTHS)]
    out += [("block/%s" % k, content(k, 65536, 40 + i), 0) for i, k in enumerate(kinds)]
    out += [("round/%s" % k, content(k, 2049, 50 + i), 0) for i, k in enumerate(kinds)]
    out.append(("every-symbol", every_symbol_block(), 0))
    out.append(("alice/30000", make_block("alice", 30000, 3), 0))
    for i, (h, body) in enumerate([(16, 5000), (16, 65520), (4080, 61456), (32752, 5002), (32752, 32784), (32768, 5004), (32768, 32768)]):
        data = make_block("lz" if i % 2 else "alice", h + body, seed=60 + i)
        out.append(("history/%d/%d" % (h, body), data, h))
    out.append(("history/16/zeros", bytes(16 + 4099), 16))
    assert all(len(d) <= 65536 and h < len(d) or not d for _, d, h in out)
    return tuple(out)
