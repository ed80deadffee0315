"""GPU tests of the output-size queries (include/nxz_engine.h: nxz_batch_decompress_size / _size_framed; the walk in
power-gzip_amd/csrc/nxz_inflate_size.hip).  Expected values come from the CPU oracle (tests/oracle_lib.py inflate) or from zlib,
never from the engine's own decode -- except in the two-pass test, which pins that the size pass and the decode pass agree."""
import ctypes as C
import importlib
import random
import struct
import threading
import time
import zlib

import numpy as np
import pytest

import framing as F
import oracle_lib as O
from datagen import make_block
from deflate_handmade import fib_table, hand_table

pytestmark = pytest.mark.gpu
pkg = importlib.import_module("power-gzip_amd")
NO_LIMIT = 0xffffffff
KINDS = ["zeros", "text33", "lz", "random", "alice", "periodic", "binary", "sparse"]
SIZES = [0, 1, 2, 3, 257, 258, 259, 32767, 32768, 32769, 65535, 65536, 200000]


@pytest.fixture(scope="module")
def eng():
    e = pkg.Engine(0)
    yield e
    e.close()


def raw(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, flush_every=0):
    co = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
    if not flush_every:
        return co.compress(data) + co.flush()
    out = b""
    for i in range(0, len(data), flush_every):
        out += co.compress(data[i:i + flush_every]) + co.flush(zlib.Z_FULL_FLUSH)
    return out + co.flush()


def place(eng, bufs, offs=None):
    """the buffers in one device tensor, each in a 16-byte aligned slot at offs[i] bytes into it; returns (tensor, addresses)"""
    import torch
    offs = offs or [0] * len(bufs)
    at, pos = [], 0
    for b, o in zip(bufs, offs):
        at.append(pos + o)
        pos += (o + len(b) + 15 + 16) & ~15
    host = np.full(max(pos, 16), 0xa5, np.uint8)
    for b, a in zip(bufs, at):
        host[a:a + len(b)] = np.frombuffer(b, np.uint8)
    t = torch.from_numpy(host).to(eng.dev)
    return t, np.uint64(t.data_ptr()) + np.array(at, np.uint64)


def make_jobs(addrs, lens, caps, hist=0, dst=0, resume=0):
    j = np.zeros(len(lens), pkg.JOB_DTYPE)
    j["src"], j["src_len"], j["dst_cap"], j["hist_len"], j["dst"], j["resume"] = addrs, lens, caps, hist, dst, resume
    j["in_adler"] = 1
    return j


def size(eng, bufs, caps=NO_LIMIT, offs=None, hist=0, dst=0, resume=0):
    src, addrs = place(eng, bufs, offs)
    jobs = eng.to_device(make_jobs(addrs, [len(b) for b in bufs], caps, hist, dst, resume))
    return eng.results_to_host(eng.decompress_size(jobs, len(bufs)))


def want(st, src_len):
    """(cc, tpbc, spbc, subc, sfbt & 0x10f, tebc, out_dhtlen) as nxz_batch_decompress documents them for the oracle's state"""
    spbc, subc = src_len, st.out_subc
    if st.final_eob and subc > 0xfff8:                 # SUBC is a 16-bit field: whole excess bytes stay unread
        drop = (subc - 0xfff8 + 7) // 8
        spbc, subc = spbc - drop, subc - 8 * drop
    cc = st.err or (0 if st.final_eob and subc < 8 else 3)
    return cc, st.tpbc, spbc, subc, st.out_sfbt | (0x100 if st.final_eob else 0), st.out_rembytecnt, st.out_dhtlen


def check_against_oracle(r, i, src, cap, hist=b""):
    _, st = O.inflate(src, cap, hist=hist)
    cc, tpbc, spbc, subc, sfbt, rem, dhtlen = want(st, len(hist) + len(src))
    assert int(r["cc"][i]) == cc, (i, int(r["cc"][i]), cc)
    if cc in (0, 3):
        got = (int(r["tpbc"][i]), int(r["spbc"][i]), int(r["subc"][i]), int(r["sfbt"][i]) & 0x10f)
        assert got == (tpbc, spbc, subc, sfbt), (i, got, (tpbc, spbc, subc, sfbt))
        if (sfbt & 0xe) == 0x8:
            assert int(r["tebc"][i]) == rem, i
        if (sfbt & 0xe) == 0xc:
            assert int(r["sfbt"][i]) >> 16 == dhtlen, i
        assert int(r["crc"][i]) == 0 and int(r["adler"][i]) == 0, i
    return cc


def whole_streams():
    out, k = [], 0
    levels = [(0, zlib.Z_DEFAULT_STRATEGY), (1, zlib.Z_DEFAULT_STRATEGY), (6, zlib.Z_DEFAULT_STRATEGY), (9, zlib.Z_DEFAULT_STRATEGY),
              (6, zlib.Z_FIXED)]
    for n in SIZES:
        for lv, st in levels:
            for _ in range(3):
                d = make_block(KINDS[k % len(KINDS)], n, seed=k)
                out.append((d, raw(d, lv, st)))
                k += 1
    for kind in ("alice", "lz", "random"):                 # hundreds of blocks, empty stored blocks between them
        d = make_block(kind, 30000, seed=k)
        out.append((d, raw(d, 6, flush_every=100)))
        k += 1
    return out


@pytest.fixture(scope="module")
def whole():
    return whole_streams()


def test_whole_streams_no_limit_no_target(eng, whole):
    big = make_block("alice", 1 << 20, seed=77) + make_block("lz", 1 << 20, seed=78)
    cases = whole + [(big, raw(big, 6))]
    assert len(cases) >= 195 and len(big) == 2 << 20
    r = size(eng, [c for _, c in cases], offs=[i % 16 for i in range(len(cases))])
    for i, (d, c) in enumerate(cases):
        assert check_against_oracle(r, i, c, len(d)) == 0, i           # (a target of exactly the output: no token is refused)
        assert int(r["tpbc"][i]) == len(d), i


def test_batch_and_grid_edges(eng, whole):
    base = whole[::2][:70]
    assert len(base) == 70
    exp = [want(O.inflate(c, len(d))[1], len(c)) for d, c in base]
    src, addrs = place(eng, [c for _, c in base])
    lens = np.array([len(c) for _, c in base], np.uint32)
    for n in (1, 63, 64, 65, 4097):
        idx = np.arange(n) % 70
        r = eng.results_to_host(eng.decompress_size(eng.to_device(make_jobs(addrs[idx], lens[idx], NO_LIMIT)), n))
        for i in range(n):
            cc, tpbc, spbc, subc, sfbt, _, _ = exp[idx[i]]
            got = (int(r["cc"][i]), int(r["tpbc"][i]), int(r["spbc"][i]), int(r["subc"][i]), int(r["sfbt"][i]) & 0x10f)
            assert got == (cc, tpbc, spbc, subc, sfbt), (n, i)


def test_source_lengths_and_alignments(eng):
    d = make_block("alice", 20000, seed=4)
    streams = [raw(d, 6), raw(d, 6, zlib.Z_FIXED), raw(make_block("random", 2000, seed=1), 0)]
    bufs, offs = [], []
    for s in streams:
        for cut in (255, 256, 257, 511, 512, 513):
            for o in range(16):
                bufs.append(s[:cut]); offs.append(o)
        for o in range(16):
            bufs.append(s); offs.append(o)
    r = size(eng, bufs, offs=offs)
    for i, b in enumerate(bufs):
        check_against_oracle(r, i, b, 30000)


def kraft(lens):
    return sum(2.0 ** -x for x in lens if x)


def test_codes_longer_than_the_fast_tables(eng):
    """tables beyond what the kernels' fast tables index (LBITS = 11, DBITS = 9): O.dhtgen on Fibonacci-like counts (it gives
    14 and 12 bits, its longest), and a table written by hand in which both alphabets reach 15"""
    tables = []
    dht, dhtlen, codes = fib_table()
    assert max(codes.ll_len) > 11 and max(codes.d_len) > 9 and codes.d_len[0] > 9 and codes.ll_len[0] > 11
    tables.append((dht, dhtlen))
    dht, dhtlen = hand_table()
    codes = O.Codes()
    assert O.lib().nxo_dht_parse(dht, dhtlen, C.byref(codes)) == dhtlen
    assert max(codes.ll_len) == 15 and max(codes.d_len) == 15 and codes.d_len[0] == 15 and codes.ll_len[205] == 15
    assert kraft(codes.ll_len) == 1.0 and kraft(codes.d_len) == 1.0
    tables.append((dht, dhtlen))
    rnd = random.Random(8)
    bufs, plains = [], []
    for dht, dhtlen in tables:
        for n in (1, 300, 5000, 40000):
            # every byte value (long literal codes), runs and short periods (distances 1..8: long distance codes), letters
            p = bytearray(range(256)) + bytes(40) + b"abc" * 30 + b"hello" * 20 + bytes(range(200, 207)) * 2
            while len(p) < n + 450:
                p += bytes(rnd.choice(b"xwvutsrqponmlkjihgfedcba etaon" * 3 + bytes(range(97, 121)) + bytes(range(200, 207))) for _ in range(50))
                p += bytes([rnd.randrange(256)]) * rnd.randrange(3, 9)
            p = bytes(p[:n + 450])
            s, bits = O.deflate_dynamic(p, dht, dhtlen)
            assert s is not None
            assert zlib.decompressobj(-15).decompress(s) == p
            plains.append(p); bufs.append(s)
            bufs.append(s[:len(s) // 2]); plains.append(p)          # and suspended inside such a block
    r = size(eng, bufs, offs=[(5 * i) % 16 for i in range(len(bufs))])
    for i, (s, p) in enumerate(zip(bufs, plains)):
        check_against_oracle(r, i, s, len(p))


def zstreams():
    """the streams of tests/test_gpu_parity.py's suspend and damage tests, rebuilt here"""
    data = {k: make_block(k, n, seed=7) for k, n in [("alice", 65536), ("lz", 65536), ("random", 20000), ("zeros", 65536), ("text33", 3000)]}
    out = []
    for name, d in data.items():
        for level, strat in [(1, zlib.Z_DEFAULT_STRATEGY), (6, zlib.Z_DEFAULT_STRATEGY), (9, zlib.Z_DEFAULT_STRATEGY),
                             (6, zlib.Z_FIXED), (0, zlib.Z_DEFAULT_STRATEGY), (6, zlib.Z_HUFFMAN_ONLY)]:
            out.append((d, raw(d, level, strat)))
    return out


def test_suspend_state_matches_oracle(eng):
    rnd = random.Random(3)
    cases = []
    for d, c in zstreams()[:18]:
        cases.append(c[:0])
        for _ in range(5):
            cases.append(c[:rnd.randrange(0, len(c))])
    assert len(cases) == 108
    r = size(eng, cases)
    kinds = set()
    for i, c in enumerate(cases):
        assert check_against_oracle(r, i, c, 70000) == 3, i
        kinds.add(int(r["sfbt"][i]) & 0xe)
    assert kinds == {0x8, 0xa, 0xc, 0xe}                   # inside stored, fixed and dynamic blocks, and in headers


def damaged_cases():
    rnd = random.Random(11)
    base = zstreams()[:24]
    cases = []
    for k in range(420):
        d, c = base[k % len(base)]
        b = bytearray(c)
        how = k % 5
        if how == 0 and b:                                # one to three flipped bits
            for _ in range(rnd.randrange(1, 4)):
                i = rnd.randrange(len(b)); b[i] ^= 1 << rnd.randrange(8)
        elif how == 1 and len(b) > 8:                     # a damaged header region
            for i in range(rnd.randrange(1, 6)):
                b[rnd.randrange(0, min(len(b), 48))] = rnd.randrange(256)
        elif how == 2 and len(b) > 4:                     # cut and flipped
            del b[rnd.randrange(1, len(b)):]
            b[rnd.randrange(len(b))] ^= 0x40
        elif how == 3:                                    # pure noise
            b = bytearray(rnd.randbytes(rnd.randrange(1, 3000)))
        elif b:                                           # a zeroed or saturated span
            i = rnd.randrange(len(b)); n = rnd.randrange(1, 64)
            b[i:i + n] = bytes([rnd.choice([0, 0xff])]) * len(b[i:i + n])
        cases.append(bytes(b))
    return cases


def test_damaged_streams_take_the_oracles_verdict(eng):
    cases = damaged_cases()
    cap = 65536 + 4096
    states = [O.inflate(c, cap)[1] for c in cases]
    assert all(st.tpbc <= cap for st in states)            # the oracle bounds every case by itself with this cap
    r = size(eng, cases, caps=cap)
    verdicts = {}
    for i, (c, st) in enumerate(zip(cases, states)):
        cc, tpbc, spbc, subc, sfbt, _, _ = want(st, len(c))
        assert int(r["cc"][i]) == cc, (i, int(r["cc"][i]), cc)
        if not st.err:
            assert cc in (0, 3)
            assert (int(r["tpbc"][i]), int(r["subc"][i]), int(r["sfbt"][i]) & 0x10f) == (tpbc, subc, sfbt), i
        verdicts[cc] = verdicts.get(cc, 0) + 1
    assert len(verdicts) >= 4, verdicts


def test_the_cap(eng, whole):
    pick = [x for x in whole if len(x[0]) in (0, 1, 3, 258, 32768, 65536)][::2][:40]
    assert len(pick) == 40 and any(len(d) == 0 for d, _ in pick)
    bufs, caps = [], []
    for d, c in pick:
        for cap in (len(d), len(d) - 1, 0):
            if cap >= 0:
                bufs.append(c); caps.append(cap)
    r = size(eng, bufs, caps=np.array(caps, np.uint32))
    k = 0
    for d, c in pick:
        S = len(d)
        assert int(r["cc"][k]) == 0 and int(r["tpbc"][k]) == S, k
        k += 1
        if S > 0:
            assert int(r["cc"][k]) == 13, (k, S)
            assert O.inflate(c, S - 1)[1].err == 13
            k += 1
        assert int(r["cc"][k]) == (13 if S > 0 else 0), (k, S)
        k += 1
    assert k == len(bufs)


class FixedBits:
    """a fixed-code block written by hand (RFC 1951 3.2.6)"""
    LB = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
    DB = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289,
          16385, 24577]

    def __init__(self):
        self.v, self.n = 0, 0
        self.put(1, 1); self.put(1, 2)                     # BFINAL, BTYPE 01

    def put(self, val, nbits):
        self.v |= val << self.n
        self.n += nbits

    def code(self, c, nbits):                              # Huffman codes go most significant bit first
        self.put(int(format(c, "0%db" % nbits)[::-1], 2), nbits)

    def sym(self, s):
        if s < 144: self.code(0x30 + s, 8)
        elif s < 256: self.code(0x190 + s - 144, 9)
        elif s < 280: self.code(s - 256, 7)
        else: self.code(0xc0 + s - 280, 8)

    def match(self, length, dist):
        ls = max(i for i in range(29) if self.LB[i] <= length)
        self.sym(257 + ls)
        self.put(length - self.LB[ls], 0 if ls < 8 or ls == 28 else (ls - 4) >> 2)
        ds = max(i for i in range(30) if self.DB[i] <= dist)
        self.code(ds, 5)
        self.put(dist - self.DB[ds], 0 if ds < 4 else (ds - 2) >> 1)

    def done(self):
        self.sym(256)
        return self.v.to_bytes((self.n + 7) // 8, "little")


def test_distances_against_the_declared_history(eng):
    bufs, hists, legal = [], [], []
    for hist in (0, 16, 32768):
        for L in (0, 1, 5):
            reach = L + hist
            for D in sorted({reach, reach + 1, min(reach, 32768)}):
                if not 1 <= D <= 32768:                    # (the format has no such distance)
                    continue
                w = FixedBits()
                for k in range(L):
                    w.sym(65 + k)
                w.match(7, D)
                bufs.append(bytes([0x77]) * hist + w.done()); hists.append(hist); legal.append(D <= reach)
    assert sum(legal) >= 7 and legal.count(False) >= 5
    r = size(eng, bufs, hist=np.array(hists, np.uint32), offs=[i % 16 for i in range(len(bufs))])
    for i, (b, h, ok) in enumerate(zip(bufs, hists, legal)):
        cc = check_against_oracle(r, i, b[h:], 100, hist=bytes(h))
        assert cc == (0 if ok else 67), (i, cc)
    # the same legal streams through zlib with a dictionary of that length
    for i, (b, h, ok) in enumerate(zip(bufs, hists, legal)):
        if ok and h:
            assert len(zlib.decompressobj(-15, zdict=bytes(h)).decompress(b[h:])) == int(r["tpbc"][i]), i


def test_jobs_it_refuses(eng):
    s = raw(b"hello hello hello")
    r = size(eng, [s, s, bytes(32784) + s, s], hist=np.array([0, 0, 32784, 0], np.uint32), resume=np.array([0, 1, 0, 0x00e80000], np.uint32))
    assert int(r["cc"][0]) == 0 and int(r["tpbc"][0]) == 17
    for i in (1, 2, 3):
        assert r[i].tolist() == (8, 0, 0, 0, 0, 0, 0, 0), i


def test_the_2_to_the_32_edge(eng):
    """63 x 64 MiB of zeros is 0xfc000000 bytes of output (CC 0), 64 x 64 MiB is 2^32: one more than dst_cap = 0xffffffff can say
    (CC 13).  About 4 MB of source each on one wavefront; the test gives the two walks 20 seconds.
    The test prints the time the two walks took; it has not been measured on an MI355X yet (expected: well under a second)."""
    import torch
    co = zlib.compressobj(6, zlib.DEFLATED, -15)
    chunk = co.compress(bytes(1 << 26)) + co.flush(zlib.Z_FULL_FLUSH)
    do = zlib.decompressobj(-15)
    n = 0
    rest = chunk + b"\x03\x00"
    while rest:                                            # (in steps: no 64 MiB Python object)
        n += len(do.decompress(rest, 1 << 22))
        rest = do.unconsumed_tail
    assert n == 1 << 26 and do.eof
    bufs = [chunk * 63 + b"\x03\x00", chunk * 64 + b"\x03\x00"]
    src, addrs = place(eng, bufs)
    jobs = eng.to_device(make_jobs(addrs, [len(b) for b in bufs], NO_LIMIT))
    torch.cuda.synchronize(eng.dev)
    done = torch.cuda.Event()
    t0 = time.monotonic()
    res = eng.decompress_size(jobs, 2)
    done.record(torch.cuda.current_stream(eng.dev))
    while not done.query():
        assert time.monotonic() - t0 < 20, "the two walks did not end within their time limit"
    print("2^32 edge: %.3f s for both walks, %d source bytes each" % (time.monotonic() - t0, len(bufs[0])))
    r = eng.results_to_host(res)
    assert int(r["cc"][0]) == 0 and int(r["tpbc"][0]) == 63 << 26 and int(r["sfbt"][0]) == 0x100 and int(r["spbc"][0]) == len(bufs[0])
    assert int(r["cc"][1]) == 13


def test_nothing_is_written(eng, whole):
    import torch
    pick = whole[::5]
    n = len(pick)
    dst = torch.full((n * 4096 + 64,), 0xAA, dtype=torch.uint8, device=eng.dev)
    src, addrs = place(eng, [c for _, c in pick])
    daddr = np.uint64(dst.data_ptr()) + np.arange(n, dtype=np.uint64) * np.uint64(4096) + np.uint64(3)      # (misaligned on purpose)
    jobs = eng.to_device(make_jobs(addrs, [len(c) for _, c in pick], NO_LIMIT, dst=daddr))
    r = eng.results_to_host(eng.decompress_size(jobs, n))
    assert [int(x) for x in r["tpbc"]] == [len(d) for d, _ in pick]
    assert bool((dst == 0xAA).all())


def test_two_passes_end_to_end(eng):
    import torch
    rnd = random.Random(21)
    plains = [make_block(KINDS[i % len(KINDS)], rnd.choice([0, 1, 100, 3000, 20000, 65536, 70001]), seed=i) for i in range(300)]
    streams = [zlib.compress(p, [1, 6, 9][i % 3]) for i, p in enumerate(plains)]
    n = len(streams)
    src, addrs = place(eng, streams, offs=[i % 16 for i in range(n)])
    jobs = eng.to_device(make_jobs(addrs, [len(s) for s in streams], NO_LIMIT))
    # pass 1: sizes
    res1, fr1 = eng.decompress_size_framed(pkg.FMT_ZLIB, jobs, n)
    # on the device: an exclusive prefix sum of tpbc rounded up to 16, then the decode jobs
    tpbc = res1.view(torch.int32).view(n, 8)[:, 1].to(torch.int64)
    slot = (tpbc + 15) & ~15
    offs = torch.cumsum(slot, 0) - slot
    total = int((offs[-1] + slot[-1]).item())
    dst = torch.empty(max(total, 16), dtype=torch.uint8, device=eng.dev)
    j64 = jobs.clone().view(torch.int64).view(n, 6)
    j64[:, 1] = offs + dst.data_ptr()
    j64[:, 3] = tpbc                                       # dst_cap (in_crc = 0 above it)
    # pass 2: decode
    res2, fr2 = eng.decompress_framed(pkg.FMT_ZLIB, j64.view(torch.uint8).reshape(-1), n)
    r1, r2, f1, f2 = eng.results_to_host(res1), eng.results_to_host(res2), eng.frames_to_host(fr1), eng.frames_to_host(fr2)
    assert (f1["status"] == F.OK).all() and (f2["status"] == F.OK).all()
    out, o = dst.cpu().numpy(), offs.cpu().numpy()
    for i, p in enumerate(plains):
        assert int(r1["tpbc"][i]) == len(p) and out[o[i]:o[i] + len(p)].tobytes() == p, i
    for k in ("cc", "tpbc", "spbc", "subc", "sfbt"):
        assert (r1[k] == r2[k]).all(), k
    for k in ("hdr_len", "end", "check", "isize"):
        assert (f1[k] == f2[k]).all(), k


def framed_cases(dictionary):
    """(family, stream, status without a dictionary, status with `dictionary`, the plain bytes or None)"""
    plain = make_block("alice", 20000, seed=5)
    z = F.zlib_stream(plain)
    g = F.gzip_member(plain, 6, flg=F.FNAME | F.FEXTRA | F.FCOMMENT | F.FHCRC, mtime=123456789, extra=b"XY\x02\x00ab", name=b"a.txt", comment=b"hi")
    g0 = F.gzip_member(plain, 6)
    ghl = F.parse(g, F.FMT_GZIP)["hdr_len"]
    co = zlib.compressobj(6, zlib.DEFLATED, 15, 8, zlib.Z_DEFAULT_STRATEGY, dictionary)
    dplain = dictionary[-3000:] + plain[:2000] + dictionary[:1500]          # reaches into the dictionary at once
    zd = co.compress(dplain) + co.flush()
    co = zlib.compressobj(6, zlib.DEFLATED, 15, 8, zlib.Z_DEFAULT_STRATEGY, b"another dictionary")
    zo = co.compress(plain) + co.flush()
    flip = lambda b, i, m=1: b[:i] + bytes([b[i] ^ m]) + b[i + 1:]
    bad_deflate_z = z[:2] + bytes([z[2] | 6]) + z[3:]                        # BTYPE 3
    bad_deflate_g = g0[:10] + bytes([g0[10] | 6]) + g0[11:]
    cases = [
        ("z", z, F.OK, F.OK, plain), ("g", g, F.OK, F.OK, plain), ("g", g0, F.OK, F.OK, plain),
        ("z", flip(z, 1), F.BAD_HEADER, F.BAD_HEADER, None),                 # FCHECK
        ("z", bytes([z[0] ^ 1]) + z[1:], None, None, None),                  # CM != 8 (FCHECK made right below)
        ("g", g[:2] + b"\x07" + g[3:], F.BAD_METHOD, F.BAD_METHOD, None),
        ("z", zd, F.NEED_DICT, F.OK, dplain), ("z", zo, F.NEED_DICT, F.NEED_DICT, None),
        ("g", flip(g, ghl - 1), F.BAD_HCRC, F.BAD_HCRC, None),
        ("z", z[:1], F.TRUNCATED, F.TRUNCATED, None), ("g", g[:ghl - 3], F.TRUNCATED, F.TRUNCATED, None),     # inside the header
        ("z", z[:len(z) // 2], F.TRUNCATED, F.TRUNCATED, None), ("g", g[:len(g) // 2], F.TRUNCATED, F.TRUNCATED, None),   # the data
        ("z", z[:-2], F.TRUNCATED, F.TRUNCATED, None), ("g", g[:-5], F.TRUNCATED, F.TRUNCATED, None),         # the trailer
        ("z", bad_deflate_z, F.DEFLATE, F.DEFLATE, None), ("g", bad_deflate_g, F.DEFLATE, F.DEFLATE, None),
        ("g", flip(g, len(g) - 2), F.BAD_LENGTH, F.BAD_LENGTH, None),       # ISIZE
        ("z", flip(z, len(z) - 3), F.OK, F.OK, plain), ("g", flip(g, len(g) - 7, 0x80), F.OK, F.OK, plain),   # Adler-32 / CRC-32: not seen
        ("z", z + b"trailing", F.OK, F.OK, plain), ("g", g + g, F.OK, F.OK, plain),
    ]
    # CM != 8 with a right FCHECK
    cmf = (z[0] & 0xf0) | 7
    flg = z[1] & 0xe0
    flg += 31 - (cmf * 256 + flg) % 31
    cases[4] = ("z", bytes([cmf, flg]) + z[2:], F.BAD_METHOD, F.BAD_METHOD, None)
    return cases


def check_framed(eng, cases, fmt, d, dictionary, with_dict):
    streams = [c[1] for c in cases]
    n = len(streams)
    src, addrs = place(eng, streams, offs=[(3 * i) % 16 for i in range(n)])
    jobs = eng.to_device(make_jobs(addrs, [len(s) for s in streams], NO_LIMIT))
    res, fr = eng.decompress_size_framed(fmt, jobs, n, d=d if with_dict else None)
    r, f = eng.results_to_host(res), eng.frames_to_host(fr)
    for i, (fam, s, st0, st1, plain) in enumerate(cases):
        st = st1 if with_dict else st0
        assert int(f["status"][i]) == st, (fmt, with_dict, i, int(f["status"][i]), st)
        model = F.parse(s, fmt)
        for k in F.FIELDS:                                 # the header's fields as framing.py reads them
            if k != "status":
                assert int(f[k][i]) == model[k], (i, k)
        hl, tl = model["hdr_len"], 8 if model["format"] == F.FMT_GZIP else 4
        if model["status"] not in (F.OK, F.NEED_DICT) or (model["status"] == F.NEED_DICT and st != F.OK):
            assert r[i].tolist() == (8, 0, 0, 0, 0, 0, 0, 0), i              # header failures: nothing walked
            assert int(f["end"][i]) == 0
            continue
        if st in (F.OK, F.BAD_LENGTH):
            dd = zlib.decompressobj(-15, zdict=dictionary) if model["status"] == F.NEED_DICT else zlib.decompressobj(-15)
            out = dd.decompress(s[hl:])
            end = len(s) - len(dd.unused_data) + tl
            assert int(f["end"][i]) == end and int(r["tpbc"][i]) == len(out), i
            if plain is not None:
                assert out == plain
            t = s[end - tl:end]
            assert int(f["check"][i]) == (struct.unpack(">I", t)[0] if tl == 4 else struct.unpack("<I", t[:4])[0]), i
            assert int(f["isize"][i]) == (0 if tl == 4 else struct.unpack("<I", t[4:])[0]), i
            assert int(r["cc"][i]) in (0, 3) and int(r["sfbt"][i]) & 0x100, i
        elif st == F.DEFLATE:
            _, ost = O.inflate(s[hl:len(s) - tl], 70000)
            assert ost.err and int(r["cc"][i]) == ost.err, i
        else:
            assert st == F.TRUNCATED and int(f["end"][i]) == 0, i
    return f


def test_framed_statuses(eng):
    dictionary = make_block("alice", 40000, seed=9)
    d = eng.dict_create(dictionary)
    try:
        cases = framed_cases(dictionary)
        for with_dict in (False, True):
            f = check_framed(eng, cases, pkg.FMT_AUTO, d, dictionary, with_dict)
            assert [int(x) for x in f["format"]] == [F.FMT_ZLIB if c[0] == "z" else F.FMT_GZIP for c in cases]
            assert int(f["dictid"][6]) == zlib.adler32(dictionary) and int(f["dictid"][7]) == zlib.adler32(b"another dictionary")
            assert int(f["end"][20]) == len(cases[20][1]) - 8 and int(f["end"][21]) == len(cases[21][1]) // 2    # trailing bytes: end < src_len
            check_framed(eng, [c for c in cases if c[0] == "z"], pkg.FMT_ZLIB, d, dictionary, with_dict)
            gz = [c for c in cases if c[0] == "g"]
            gz.append(("g", b"\x1f\x8c" + gz[0][1][2:], F.BAD_HEADER, F.BAD_HEADER, None))                       # bad magic
            check_framed(eng, gz, pkg.FMT_GZIP, d, dictionary, with_dict)
    finally:
        torch_sync(eng)
        d.close()


def torch_sync(eng):
    eng.torch.cuda.synchronize(eng.dev)


def test_two_streams_at_once(eng, whole):
    L = eng.L
    L.nxz_stream_create.restype = C.c_void_p
    L.nxz_stream_create.argtypes = [C.c_void_p]
    L.nxz_stream_destroy.argtypes = [C.c_void_p, C.c_void_p]
    halves = [whole[0::2][:90], whole[1::2][:90]]
    work = []
    for part in halves:
        src, addrs = place(eng, [c for _, c in part])
        n = 300                                            # (long streams first: the order workspace of each stream is in use)
        idx = np.arange(n) % len(part)
        jobs = eng.to_device(make_jobs(addrs[idx], np.array([len(c) for _, c in part], np.uint32)[idx], NO_LIMIT))
        res = eng.torch.empty(n * pkg.RESULT_DTYPE.itemsize, dtype=eng.torch.uint8, device=eng.dev)
        work.append((src, jobs, res, n, idx, part))
    torch_sync(eng)
    handles = [L.nxz_stream_create(eng.ctx) for _ in range(2)]
    assert all(handles)
    rcs = [None, None]

    def run(k):
        src, jobs, res, n, idx, part = work[k]
        rc = 0
        for _ in range(4):
            rc = rc or L.nxz_batch_decompress_size(eng.ctx, jobs.data_ptr(), n, res.data_ptr(), C.c_void_p(handles[k]))
        rcs[k] = rc or L.nxz_ctx_sync(eng.ctx, C.c_void_p(handles[k]))
    threads = [threading.Thread(target=run, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert rcs == [0, 0]
    for k in range(2):
        src, jobs, res, n, idx, part = work[k]
        r = eng.results_to_host(res)
        for i in range(n):
            d, c = part[idx[i]]
            assert int(r["cc"][i]) == 0 and int(r["tpbc"][i]) == len(d) and int(r["spbc"][i]) == len(c), (k, i)
    for h in handles:
        L.nxz_stream_destroy(eng.ctx, C.c_void_p(h))
