"""Blocks and target sizes for the compress side's output edges (tests/test_gpu_compress_edges.py part A; the coverage is
checked on the CPU by tests/test_compress_edge_cases_host.py).  The truth is always the oracle's: LZ77 + the fixed code, a
caller's table or the table nxo_dhtgen makes of the block's own counts.

An emitter is one way the engine writes a block; a class is what its expected bytes depend on (which code, how much history).
Every class has the sizes 0, 1, 7, 64, about 1000, 2049 (one position past the entropy kernel's round of 2048) and 16385 (one past
the LZ77 tile), and a few blocks more, picked so that the class has every L % 4 (L the output length), an end-of-block code that
straddles a dword, a block that ends exactly on a dword and, for the dynamic codes, an empty block whose header alone is longer
than a dword."""
import ctypes as C
import functools
import json
import os

import numpy as np

import oracle_lib as O
from datagen import make_block

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (0, 1, 7, 64, 1000, 2049, 16385)
DICT = make_block("text33", 1000, seed=77)                   # its deflate window: the last 992 bytes

# class -> (code, history): "fixed", "canned" (tests/golden/builtin_dht.json, table 0), "own" (nxo_dhtgen of the block's counts);
# history > 0: that many bytes in front of the block; "dict": DICT's deflate window
CLASSES = {"fixed": ("fixed", 0), "fixed/16": ("fixed", 16), "fixed/32768": ("fixed", 32768), "canned": ("canned", 0),
           "own": ("own", 0), "own/dict": ("own", "dict")}
# emitter -> (function code, class, environment, through nxz_batch_compress_dict)
EMITTERS = {
    "FHT": ("FHT", "fixed", {}, False),
    "FHT_COUNT": ("FHT_COUNT", "fixed", {}, False),
    "RESUME_FHT/16": ("RESUME_FHT", "fixed/16", {}, False),
    "RESUME_FHT/32768": ("RESUME_FHT", "fixed/32768", {}, False),
    "DHT": ("DHT", "canned", {}, False),
    "DHTGEN": ("DHTGEN", "own", {"NXZ_FUSED_GEN": "0"}, False),
    "DHTGEN_COUNT": ("DHTGEN_COUNT", "own", {}, False),
    "DHTGEN/fused": ("DHTGEN", "own", {"NXZ_FUSED_GEN": "1"}, False),
    "DHTGEN/dict": ("DHTGEN", "own/dict", {}, True),
}

# class -> (kind, n, seed) of make_block: the sizes above, then the blocks that complete the coverage
_SIZED = (("lz", 0, 1), ("lz", 1, 1), ("text33", 7, 1), ("text33", 64, 1), ("lz", 1000, 1), ("random", 2049, 1), ("lz", 16385, 1))
BLOCKS = {
    "fixed": _SIZED + (("random", 996, 1), ("lz", 1004, 3)),
    "fixed/16": _SIZED + (("random", 996, 1), ("lz", 1004, 3)),
    "fixed/32768": _SIZED + (("lz", 996, 1),),
    "canned": _SIZED + (("text33", 999, 1),),
    "own": _SIZED + (("text33", 996, 2),),
    "own/dict": _SIZED + (("lz", 996, 2), ("random", 997, 3)),
}


@functools.lru_cache(maxsize=None)
def canned_table():
    g = json.load(open(os.path.join(ROOT, "tests", "golden", "builtin_dht.json")))
    return bytes.fromhex(g[0]["dht"]), g[0]["dhtlen"]


def dict_window():
    w = min(len(DICT), 32768) & ~15
    return DICT[len(DICT) - w:]


def history(cls):
    h = CLASSES[cls][1]
    if h == "dict":
        return dict_window()
    return make_block("text33", 32768, seed=5)[32768 - h:] if h else b""


class Case:
    """one block of a class with what the oracle makes of it"""

    def __init__(self, cls, kind, n, seed):
        self.cls, self.name = cls, "%s/%s/%d/%d" % (cls, kind, n, seed)
        self.body = make_block(kind, n, seed=seed)
        self.hist = history(cls)
        self.data = self.hist + self.body                        # what the oracle sees: [history][block]
        code = CLASSES[cls][0]
        tok, nt = O.lz77(self.data, len(self.hist))
        ll, d = O.counts(tok, nt)
        self.counts = np.array(list(ll) + list(d), np.uint32)
        if code == "fixed":
            self.exp, self.bits = O.deflate_fixed(self.data, len(self.hist))
            self.eob_len, self.header_bits = 7, 3
        else:
            dht, dhtlen = O.dhtgen(ll, d) if code == "own" else canned_table()
            cap = 2 * len(self.data) + 2048
            buf = C.create_string_buffer(cap)
            self.bits = O.lib().nxo_encode_dynamic(tok, nt, dht, dhtlen, buf, cap)
            self.exp = buf.raw[:(self.bits + 7) // 8] if self.bits < (1 << 62) else None     # None: the table misses a symbol
            codes = O.Codes()
            O.lib().nxo_dht_parse(dht, dhtlen, C.byref(codes))
            self.eob_len, self.header_bits = int(codes.ll_len[256]), 3 + dhtlen
        if self.exp is not None:
            self.L = len(self.exp)
            self.tebc = self.bits % 8
            self.cc = 64 if self.L > len(self.data) else 0       # NXZ_CC_TPBC_GT_SPBC: more bytes out than in (history counts)
            before = self.bits - self.eob_len                    # bits in front of the end-of-block code
            self.straddles = before % 32 + self.eob_len > 32
            self.dword_exact = self.bits % 32 == 0

    def caps(self):
        """{0, 1, 3, 4, L-5 .. L+4, L & ~3, (L & ~3) + 4}, clipped at 0"""
        L = self.L
        return sorted({c for c in [0, 1, 3, 4, L & ~3, (L & ~3) + 4] + list(range(L - 5, L + 5)) if c >= 0})


@functools.lru_cache(maxsize=None)
def cases(cls):
    return tuple(Case(cls, kind, n, seed) for kind, n, seed in BLOCKS[cls])


def coverage(cs):
    """what a set of cases covers: the classes of part A"""
    return {"sizes": {len(c.body) for c in cs}, "mod4": {c.L % 4 for c in cs}, "straddle": sum(c.straddles for c in cs),
            "dword_exact": sum(c.dword_exact for c in cs),
            "empty_header_bits": [c.header_bits for c in cs if not c.body]}


WRAP_SIZES = (0, 1, 15, 16, 17, 4097)
