"""The rules of nxz_batch_deflate_streams_indexed (power-gzip_amd/csrc/nxz_streams_index.h: the block headers of a piece, the sentinel,
rule 2 over the headers in stream order) -- the code the kernels of nxz_streams_index.hip run -- compiled for the host under
AddressSanitizer and UBSan (tests/native/streams_index_host.cpp).  Held against a plain-Python restatement of the rules for random
piece lists, and against zlib itself (tests/checkpoint_model.py: inflate with Z_BLOCK) for streams whose bytes Python writes the way
pack_block lays them out: stored pieces, and pieces that zlib compressed to one block each."""
import os
import random
import struct
import subprocess
import zlib

import pytest

import checkpoint_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RAW, ZLIB, GZIP = 0, 1, 2
HDR = {RAW: b"", ZLIB: b"\x78\x9c", GZIP: bytes.fromhex("1f8b0800000000000403")}
OK, MORE = 0, 2                                      # NXZ_CPS_OK, NXZ_CPS_MORE
BIG = 1 << 31                                        # a cp_cap no list here reaches


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    exe = tmp_path_factory.mktemp("streams_index") / "streams_index_host"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "power-gzip_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "streams_index_host.cpp"), "-o", str(exe)], check=True)

    def run(lines):
        r = subprocess.run([str(exe)], input=("\n".join(lines) + "\n").encode(), capture_output=True, timeout=600)
        assert r.returncode == 0, r.stderr.decode()[-4000:]
        return r.stdout.decode().splitlines()
    return run


def ask(host, cases):
    """cases: [(hdr_len, span, cp_cap, pieces)] -> one dict per case: H, C, S, count, status, bytes"""
    lines = []
    for hdr_len, span, cp_cap, pieces in cases:
        lines.append("run %d %d %d %d" % (hdr_len, span, cp_cap, len(pieces)))
        lines += ["%d %d %d %d %d" % p for p in pieces]
    out, got, cur = host(lines), [], None
    for line in out:
        if cur is None:
            cur = {"H": [], "C": [], "S": None}
        f = line.split()
        if f[0] == "H":
            cur["H"].append((int(f[1]), int(f[2])))
        elif f[0] == "C":
            cur["C"].append((int(f[1]), int(f[2]), int(f[3])))
        elif f[0] == "S":
            cur["S"] = (int(f[1]), int(f[2]))
        elif f[0] == "N":
            cur["count"], cur["status"] = int(f[1]), int(f[2])
        elif f[0] == "E":
            cur["bytes"] = int(f[1])
        else:
            assert f[0] == "."
            got.append(cur)
            cur = None
    assert len(got) == len(cases)
    return got


def model(hdr_len, span, cp_cap, pieces):
    """the issue's rules, restated: pieces (stored, len, keep, tebc, final) laid one behind the other behind hdr_len bytes"""
    P, u0, H = hdr_len, 0, []
    end = 8 * hdr_len + 40
    if not pieces:
        H.append((8 * hdr_len, 0))
        P += 5
    for stored, ln, keep, tebc, final in pieces:
        H.append((8 * P, u0))
        if stored:
            size = ln + 10 if ln > 65535 else ln + 5
            if ln > 65535:
                H.append((8 * (P + 5 + 65535), u0 + 65535))
            end = 8 * (P + size)
        else:
            marker = not final and tebc != 0
            size = keep + ((1 if tebc + 3 > 8 else 0) + 4 if marker else 0)
            if marker:
                H.append((8 * (P + keep - 1) + tebc, u0 + ln))
            end = 8 * (P + keep - 1) + (tebc if tebc else 8)
        P += size
        u0 += ln
    C, c = [], 0
    for n, (bit, u) in enumerate(H):
        if n == 0 or u - c >= span:
            C.append((min(len(C), cp_cap), bit, u))
            c = u
    count = len(C)
    return {"H": H, "C": C, "S": (end, u0) if count <= cp_cap else None, "count": count, "status": MORE if count > cp_cap else OK, "bytes": P}


def random_pieces(rnd, B, n, force=None):
    out = []
    for k in range(n):
        final = k == n - 1
        ln = B if not final else rnd.choice([1, 15, 16, B - 1, B, 65535 if B >= 65535 else B, B])
        if rnd.random() < 0.3:
            out.append((1, ln, 0, 0, int(final)))
        else:
            tebc = rnd.randrange(8) if force is None else force
            out.append((0, ln, rnd.randrange(1, ln + 1), tebc, int(final)))
    return out


@pytest.mark.parametrize("B", [65536, 61440, 32768])
def test_random_piece_lists_against_the_rules_restated(host, B):
    rnd = random.Random(B)
    cases = []
    for span in (1, B, B + 1, 3 * B, 2 ** 40):
        for hdr_len in (0, 2, 10):
            cases.append((hdr_len, span, BIG, []))                                        # the empty buffer
            for tebc in range(8):                                                        # a single piece, and every tebc in a list
                cases.append((hdr_len, span, BIG, [(0, 100, 40, tebc, 1)]))
                cases.append((hdr_len, span, BIG, random_pieces(rnd, B, 5, force=tebc)))
            cases.append((hdr_len, span, BIG, [(1, 100, 0, 0, 1)]))
            if B == 65536:                                                               # stored pieces of 65535 and 65536 bytes
                cases.append((hdr_len, span, BIG, [(1, 65536, 0, 0, 0), (1, 65535, 0, 0, 1)]))
                cases.append((hdr_len, span, BIG, [(1, 65536, 0, 0, 0), (0, 65536, 9, 3, 0), (1, 65536, 0, 0, 1)]))
            for _ in range(6):
                cases.append((hdr_len, span, BIG, random_pieces(rnd, B, rnd.randrange(1, 140))))
    for (hdr_len, span, cp_cap, pieces), got in zip(cases, ask(host, cases)):
        assert got == model(hdr_len, span, cp_cap, pieces), (hdr_len, span, pieces[:4])


def test_cp_cap_stores_some_and_counts_all(host):
    rnd = random.Random(5)
    pieces = random_pieces(rnd, 65536, 40)
    full = model(2, 65536, BIG, pieces)
    count = full["count"]
    assert count > 3
    cases = [(2, 65536, cap, pieces) for cap in (1, count - 1, count, count + 1)]
    for (hdr_len, span, cap, _), got in zip(cases, ask(host, cases)):
        assert got == model(hdr_len, span, cap, pieces)
        assert got["count"] == count and [c[1:] for c in got["C"]] == [c[1:] for c in full["C"]]
        assert [c[0] for c in got["C"]] == [min(k, cap) for k in range(count)]
        assert (got["status"], got["S"]) == ((MORE, None) if cap < count else (OK, full["S"]))


def test_a_marker_is_taken_before_the_header_behind_it(host):
    # two pieces of B bytes, the first ends inside a byte: its marker and the second piece's header both have u = B
    B = 65536
    got = ask(host, [(0, B, BIG, [(0, B, 1000, 5, 0), (0, B, 500, 0, 1)])])[0]
    assert got["H"] == [(0, 0), (8 * 999 + 5, B), (8 * 1004, B)]
    assert got["C"] == [(0, 0, 0), (1, 8 * 999 + 5, B)] and got["S"] == (8 * (1004 + 500), 2 * B)
    # tebc 6: the three header bits of the empty block spill into a pad byte
    got = ask(host, [(0, B, BIG, [(0, B, 1000, 6, 0), (0, B, 500, 3, 1)])])[0]
    assert got["H"] == [(0, 0), (8 * 999 + 6, B), (8 * 1005, B)] and got["S"] == (8 * (1005 + 499) + 3, 2 * B)
    assert host(["size 0 65536 1000 6 0", "size 0 65536 1000 5 0", "size 0 65536 1000 0 0", "size 0 65536 1000 5 1", "size 1 65536 0 0 0",
                 "size 1 65535 0 0 1"]) == ["1005", "1004", "1000", "1000", "65546", "65540"]


def test_shape(host):
    assert host(["shape 0 1", "shape 1 %d" % (2 ** 32 - 2), "shape 1 %d" % (2 ** 32 - 1), "shape 65536 65535", "shape 65536 65534",
                 "shape %d 1" % (2 ** 31 - 1), "shape %d 1" % 2 ** 31]) == ["1", "1", "0", "0", "1", "1", "0"]


# ---- against zlib: the bytes as pack_block lays them out (nxz_pack_block.h) ------------------------------------------------------------
def stored_piece(data, final):
    first, rest = data[:65535], data[65535:]
    out = bytes([1 if final and not rest else 0]) + struct.pack("<HH", len(first), len(first) ^ 0xffff) + first
    if len(data) > 65535:
        out += bytes([1 if final else 0]) + struct.pack("<HH", len(rest), len(rest) ^ 0xffff) + rest
    return out


def compressed_piece(data, final):
    """one deflate block from zlib, then what pack_block does with a compress job's output -> (bytes, keep, tebc)"""
    raw = M.deflate(data, RAW)
    headers, end, plain = M.block_boundaries(raw, RAW)
    assert len(headers) == 1 and plain == data            # (zlib wrote ONE block, BFINAL set, as the entropy kernel does)
    keep, tebc = (end[0] + 7) // 8, end[0] % 8
    b = bytearray(raw[:keep])
    b[0] = (b[0] & ~1) | (1 if final else 0)
    if tebc:
        b[-1] &= (1 << tebc) - 1
    if not final and tebc:
        b += (b"\x00" if tebc + 3 > 8 else b"") + b"\x00\x00\xff\xff"
    return bytes(b), keep, tebc


def frame(fmt, body, data):
    if fmt == ZLIB:
        return HDR[fmt] + body + struct.pack(">I", zlib.adler32(data))
    if fmt == GZIP:
        return HDR[fmt] + body + struct.pack("<II", zlib.crc32(data), len(data) & 0xffffffff)
    return body


def check_against_zlib(host, fmt, parts, kinds, spans):
    """parts: the pieces' source bytes; kinds[k]: stored or not"""
    body, pieces = b"", []
    for k, (d, stored) in enumerate(zip(parts, kinds)):
        final = k == len(parts) - 1
        if stored:
            body += stored_piece(d, final)
            pieces.append((1, len(d), 0, 0, int(final)))
        else:
            b, keep, tebc = compressed_piece(d, final)
            body += b
            pieces.append((0, len(d), keep, tebc, int(final)))
    data = b"".join(parts)
    stream = frame(fmt, body if parts else bytes.fromhex("010000ffff"), data)
    assert zlib.decompress(stream, M.WBITS[fmt]) == data
    headers, end, _ = M.block_boundaries(stream, fmt)
    got = ask(host, [(len(HDR[fmt]), span, BIG, pieces) for span in spans])
    for span, g in zip(spans, got):
        idx = M.index(stream, fmt, span)
        assert g["H"] == headers and g["S"] == end, (fmt, span)
        assert [c[1] for c in g["C"]] + [g["S"][0]] == idx["cbit"] and [c[2] for c in g["C"]] + [g["S"][1]] == idx["uoff"], (fmt, span)
        assert g["count"] == idx["count"] and g["bytes"] == len(stream) - {RAW: 0, ZLIB: 4, GZIP: 8}[fmt]
    return pieces


@pytest.mark.parametrize("fmt", [RAW, ZLIB, GZIP])
def test_stored_pieces_against_zlib(host, fmt):
    rnd = random.Random(fmt)
    B = 65536
    spans = [1, B, B + 1, 3 * B, 2 ** 40]
    for lens in ([], [1], [65535], [65536], [B, B, 65535], [B, B, B, B, 17], [B] * 7 + [B]):
        parts = [rnd.randbytes(n) for n in lens]
        check_against_zlib(host, fmt, parts, [True] * len(parts), spans)
    B = 32768                                                  # hist_max 32768: no piece has a second stored block
    parts = [rnd.randbytes(n) for n in [B] * 5 + [100]]
    check_against_zlib(host, fmt, parts, [True] * len(parts), [1, B, B + 1, 3 * B])


@pytest.mark.parametrize("fmt", [RAW, ZLIB, GZIP])
def test_compressed_pieces_against_zlib(host, fmt):
    """pieces of a few hundred bytes stand for blocks of B: the rules take any len.  Markers of every tebc that turns up, markers
    beside stored pieces, a final piece that ends inside a byte."""
    rnd = random.Random(10 + fmt)
    words = [bytes(rnd.choice(b"abcdefgh ") for _ in range(rnd.randrange(2, 9))) for _ in range(50)]
    seen = set()
    for trial in range(12):
        parts, kinds = [], []
        for _ in range(rnd.randrange(1, 12)):
            stored = rnd.random() < 0.25
            parts.append(rnd.randbytes(rnd.randrange(1, 400)) if stored else b"".join(rnd.choice(words) for _ in range(rnd.randrange(1, 120))))
            kinds.append(stored)
        n = sum(len(p) for p in parts)
        pieces = check_against_zlib(host, fmt, parts, kinds, [1, 200, n // 3 + 1, 2 ** 40])
        seen |= {p[3] for p in pieces[:-1] if not p[0]}
    assert len(seen) >= 6 and 0 in seen, seen                  # (markers at most bit positions, and pieces that end on a byte)
