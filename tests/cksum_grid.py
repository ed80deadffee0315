"""The cases the block checksums are pinned on, shared by the host test of the slice arithmetic
(test_cksum_slices_host.py) and the GPU test of the entropy kernel (test_gpu_encode_cksum.py): source lengths round
the slice (64), pair-of-slices (128), round (2048), tile (16384) and block (65536) edges, histories in front (16-byte
multiples, as the engine's callers give them), seeds, and data that drives the Adler sums to their largest."""
import zlib

import numpy as np

LENGTHS = (0, 1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 2047, 2048, 2049, 16383, 16384, 65535, 65536)
HISTORIES = (0, 16, 48, 32768)
BLOCK = 65536


def legal_adler(v):
    return ((((v >> 16) & 0xffff) % 65521) << 16) | ((v & 0xffff) % 65521)


def seeds():
    rng = np.random.default_rng(13)
    return ((0, 1), (0xffffffff, legal_adler(0xfff0fff0)),
            (int(rng.integers(0, 1 << 32)), legal_adler(int(rng.integers(0, 1 << 32)))))


def cases():
    """[(h, n, in_crc, in_adler, bytes of history + source)], the same list on every call"""
    rng = np.random.default_rng(1313)
    out = []
    for kind in ("random", "zeros", "ff"):
        for n in LENGTHS:
            for h in HISTORIES:
                if h + n > BLOCK:
                    continue
                for in_crc, in_adler in seeds():
                    if kind == "random":
                        buf = rng.integers(0, 256, h + n, dtype=np.uint8).tobytes()
                    else:
                        # (the history is never what the source is: a checksum that took a history byte in would show)
                        buf = rng.integers(1, 255, h, dtype=np.uint8).tobytes() + (b"\x00" if kind == "zeros" else b"\xff") * n
                    out.append((h, n, in_crc, in_adler, buf))
    return out


def expected(case):
    h, n, in_crc, in_adler, buf = case
    return zlib.crc32(buf[h:], in_crc) & 0xffffffff, zlib.adler32(buf[h:], in_adler) & 0xffffffff
