"""The rules of the output-size query (power-gzip_amd/csrc/nxz_size.h: does a token still fit dst_cap, may a distance reach that
far, what goes into the result record at each kind of stop) -- the code the size kernel runs -- compiled for the host under
AddressSanitizer and UBSan (tests/native/size_host.cpp).  The fit and the distance are held against plain integer arithmetic in
Python (no 32-bit wrap), the record against what the oracle (oracle/nxz_inflate.c) reports for real streams: whole, cut,
capped and damaged."""
import os
import subprocess
import zlib

import pytest

import oracle_lib as O
from datagen import make_block

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M32 = 0xffffffff


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    exe = tmp_path_factory.mktemp("size") / "size_host"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "power-gzip_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "size_host.cpp"), "-o", str(exe)], check=True)

    def run(lines):
        r = subprocess.run([str(exe)], input=("\n".join(lines) + "\n").encode(), capture_output=True, timeout=600)
        assert r.returncode == 0, r.stderr.decode()[-4000:]
        out = r.stdout.decode().splitlines()
        assert len(out) == len(lines)
        return out
    return run


def test_fit_rule_has_no_32_bit_wrap(host):
    caps = [0, 1, 257, 258, 0xfffffffe, M32]
    produced = [0, 1, 2, 256, 257, 258, 259, 1 << 31, M32 - 258, M32 - 257, M32 - 2, M32 - 1, M32]
    lens = [0, 1, 2, 3, 257, 258, 65535]
    cases = [(p, n, c) for c in caps for p in produced for n in lens]
    out = host(["fit %d %d %d" % c for c in cases])
    for (p, n, c), line in zip(cases, out):
        assert int(line) == (1 if p + n <= c else 0), (p, n, c)
    # the pairs a wrapped 32-bit sum would get wrong are among them
    assert any(((p + n) & M32) <= c < p + n for p, n, c in cases)


def test_distance_rule(host):
    cases = []
    for hist in (0, 16, 32768):
        for produced in (0, 1, 5, 257, 32767, 32768, 65536, M32 - 1, M32, (1 << 32) + 70000):
            reach = produced + hist
            for dist in (reach - 1, reach, reach + 1):
                if 1 <= dist <= M32:
                    cases.append((dist, produced, hist))
    out = host(["dist %d %d %d" % c for c in cases])
    for (dist, produced, hist), line in zip(cases, out):
        assert int(line) == (1 if dist <= produced + hist else 0), (dist, produced, hist)
    assert sum(int(x) for x in out) not in (0, len(out))


def test_jobs_it_refuses_and_the_history_it_skips(host):
    cases = [(0, 0, 100), (0, 16, 100), (0, 32768, 40000), (0, 32768, 100), (0, 32769, 40000), (0, 32784, 40000), (1, 0, 100),
             (0x00e80000, 0, 100), (0, M32, 100), (0, 50, 50), (0, 50, 0)]
    out = host(["job %d %d %d" % c for c in cases])
    for (resume, hist_len, src_len), line in zip(cases, out):
        ok, hb = [int(x) for x in line.split()]
        assert ok == (1 if resume == 0 and hist_len <= 32768 else 0), (resume, hist_len)
        assert hb == min(hist_len, src_len)
    assert host(["refused"])[0] == "8 0 0 0 0 0 0 0"


def _streams():
    out = []
    for kind, n in (("alice", 40000), ("lz", 65536), ("random", 3000), ("zeros", 65536), ("text33", 0), ("text33", 1)):
        d = make_block(kind, n, seed=3)
        for level, strat in ((6, zlib.Z_DEFAULT_STRATEGY), (0, zlib.Z_DEFAULT_STRATEGY), (6, zlib.Z_FIXED)):
            co = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strat)
            out.append((d, co.compress(d) + co.flush()))
    return out


def _expect(st, src_len):
    """the record nxz_batch_decompress documents for the oracle's state (include/nxz_engine.h; tests/test_gpu_parity.py)"""
    spbc, subc = src_len, st.out_subc
    if st.final_eob and subc > 0xfff8:                 # SUBC is a 16-bit field: whole excess bytes stay unread
        drop = (subc - 0xfff8 + 7) // 8
        spbc -= drop
        subc -= 8 * drop
    cc = st.err or (0 if st.final_eob and subc < 8 else 3)
    sfbt = st.out_sfbt | (0x100 if st.final_eob else 0)
    if (st.out_sfbt & 0xe) == 0xc and st.out_dhtlen:
        sfbt |= st.out_dhtlen << 16
    return cc, (st.tpbc if cc in (0, 3) else 0), st.out_rembytecnt, spbc, 0, 0, subc, sfbt


def test_the_record_at_each_stop_is_the_oracles(host):
    import random
    rnd = random.Random(5)
    cases = []                                           # (source, cap)
    for d, c in _streams():
        cases.append((c, len(d)))                        # the final EOB at the end of the source: CC 0
        cases.append((c + b"12345678", len(d)))          # a trailer behind it: CC 3, sfbt 0, subc 64
        cases.append((c + bytes(9000), len(d) + 1))      # more behind it than SUBC can say
        if len(d):
            cases.append((c, len(d) - 1))                # CC 13
        for _ in range(4):                               # the source runs out: in a header, a table, a stored or coded block
            cases.append((c[:rnd.randrange(0, len(c))], len(d)))
        b = bytearray(c)
        if b:
            b[rnd.randrange(len(b))] ^= 1 << rnd.randrange(8)
            cases.append((bytes(b), 70000))              # damage: an error code, or a stream that decodes to something else
    lines, want = [], []
    for src, cap in cases:
        _, st = O.inflate(src, cap)
        have_dht = 1 if st.out_dhtlen else 0
        if st.err:                                       # the walk reports an error from a clean stop state
            lines.append("rec %d 0 %d 0 0 0 %d %d %d" % (st.err, st.tpbc, have_dht, st.out_dhtlen, len(src)))
            want.append((st.err, 0, 0, len(src), 0, 0, 0, 0))
        else:
            lines.append("rec 0 %d %d %d %d %d %d %d %d" % (st.final_eob, st.tpbc, st.out_sfbt, st.out_subc, st.out_rembytecnt,
                                                            have_dht, st.out_dhtlen, len(src)))
            want.append(_expect(st, len(src)))
    out = host(lines)
    kinds = set()
    for line, w, ln in zip(out, want, lines):
        assert tuple(int(x) for x in line.split()) == w, (ln, line, w)
        kinds.add((w[0], w[7] & 0xe, bool(w[7] & 0x100)))
    # every kind of stop occurred: final (CC 0 and CC 3), stored / fixed / dynamic / header suspends, CC 13 and a data error
    assert {(0, 0, True), (3, 0, True), (3, 0x8, False), (3, 0xa, False), (3, 0xc, False), (3, 0xe, False)} <= kinds, kinds
    assert any(k[0] == 13 for k in kinds) and any(k[0] in (66, 67, 68) for k in kinds), kinds
    # the table length travels only with a suspend inside a dynamic block
    assert any((w[7] >> 16) for w in want) and all((w[7] >> 16) == 0 for w in want if (w[7] & 0xe) != 0xc)
