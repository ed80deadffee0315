"""GPU tests of the batched verify (include/nxz_engine.h: nxz_batch_decompress_verify / _verify_framed; the kernel in
power-gzip_amd/csrc/nxz_inflate_verify.hip): checksums and trailer checks with dst = NULL in every job.  The yardsticks are zlib
(crc32 / adler32 of the plain bytes), the CPU oracle (tests/oracle_lib.py inflate) and the existing calls -- the size calls for every
field but the checksums, the decoding calls into real targets for the framed records -- never the new call's own output."""
import ctypes as C
import importlib
import os
import random
import struct
import threading
import zlib

import numpy as np
import pytest

import checkpoint_build_cases as B
import checkpoint_fine_model as M
import framing as F
import oracle_lib as O
from datagen import make_block

pytestmark = pytest.mark.gpu
pkg = importlib.import_module("power-gzip_amd")
KNOBS = ("NXZ_INFLATE_LANES_MIN", "NXZ_INFLATE_CUT", "NXZ_INFLATE_WG", "NXZ_INFLATE_WG_MAX", "NXZ_WG_PMIN", "NXZ_INFLATE_ORDER",
         "NXZ_BGZF_CHUNK", "NXZ_STREAMS_CHUNK")
NO_LIMIT = 0xffffffff
PASS = 16384                                               # nxz_verify.h: the output between two checksum passes at most
KINDS = ["zeros", "text33", "lz", "random", "alice", "periodic", "binary", "sparse"]
SIZES = [0, 1, 63, 64, 65, PASS - 1, PASS, PASS + 1, 32767, 32768, 32769, 65535, 65536, 200000]
REFUSED = (8, 0, 0, 0, 0, 0, 0, 0)
RECORD = ("cc", "tpbc", "tebc", "spbc", "subc", "sfbt")    # what the size call specifies for cc 0 and 3
POISON = 0xA5


@pytest.fixture(scope="module")
def eng():
    saved = {k: os.environ.pop(k, None) for k in KNOBS}
    e = pkg.Engine(0)
    yield e
    e.close()
    for k, v in saved.items():
        if v is not None:
            os.environ[k] = v


def raw(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, zdict=None):
    co = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy, zdict) if zdict is not None else zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
    return co.compress(data) + co.flush()


def place(eng, bufs, offs=None):
    """the buffers in one device tensor, each in a 16-byte aligned slot at offs[i] bytes into it; returns (tensor, addresses)"""
    import torch
    offs = offs or [0] * len(bufs)
    at, pos = [], 0
    for b, o in zip(bufs, offs):
        at.append(pos + o)
        pos += (o + len(b) + 15 + 16) & ~15
    host = np.full(max(pos, 16), POISON, np.uint8)
    for b, a in zip(bufs, at):
        host[a:a + len(b)] = np.frombuffer(b, np.uint8)
    t = torch.from_numpy(host).to(eng.dev)
    return t, np.uint64(t.data_ptr()) + np.array(at, np.uint64)


def make_jobs(addrs, lens, caps=NO_LIMIT, hist=0, dst=0, resume=0, in_crc=0, in_adler=1, reserved=0):
    j = np.zeros(len(lens), pkg.JOB_DTYPE)
    j["src"], j["src_len"], j["dst_cap"], j["hist_len"], j["dst"], j["resume"] = addrs, lens, caps, hist, dst, resume
    j["in_crc"], j["in_adler"], j["reserved"] = in_crc, in_adler, reserved
    return j


def targets(eng, addrs_of, caps):
    """a copy of the jobs with real targets of caps[i] bytes each: (tensor, host jobs)"""
    import torch
    pos, at = 0, []
    for c in caps:
        at.append(pos)
        pos += (int(c) + 31) & ~15
    t = torch.full((pos + 16,), POISON, dtype=torch.uint8, device=eng.dev)
    j = addrs_of.copy()
    j["dst"] = np.uint64(t.data_ptr()) + np.array(at, np.uint64)
    j["dst_cap"] = np.array(caps, np.uint32)
    return t, j


def guarded(eng, n, dtype):
    """n records inside a poisoned array, 64 guard bytes on both sides: (whole tensor, the records' view)"""
    import torch
    whole = torch.full((n * dtype.itemsize + 128,), POISON, dtype=torch.uint8, device=eng.dev)
    return whole, whole[64:64 + n * dtype.itemsize]


def guards_intact(whole):
    h = whole.cpu().numpy()
    return bool((h[:64] == POISON).all() and (h[-64:] == POISON).all())


def run_raw(eng, bufs, offs=None, **fields):
    """the verify call and the size call on the same jobs (dst = NULL): (verify records, size records); the records sit between
    guard bytes and the source must come back unchanged"""
    n = len(bufs)
    src, addrs = place(eng, bufs, offs)
    before = src.clone()
    jobs = eng.to_device(make_jobs(addrs, [len(b) for b in bufs], **fields))
    whole, res = guarded(eng, n, pkg.RESULT_DTYPE)
    v = eng.results_to_host(eng.decompress_verify(jobs, n, res)).copy()
    s = eng.results_to_host(eng.decompress_size(jobs, n))
    assert guards_intact(whole) and bool((src == before).all())
    return v, s


def same_record(v, s, i, what=""):
    """every field but the checksums is the size call's (cc 0 and 3); elsewhere only cc is specified"""
    assert int(v["cc"][i]) == int(s["cc"][i]), (what, i, int(v["cc"][i]), int(s["cc"][i]))
    if int(s["cc"][i]) in (0, 3):
        for k in RECORD:
            assert int(v[k][i]) == int(s[k][i]), (what, i, k, int(v[k][i]), int(s[k][i]))


def sums_are(v, i, plain, in_crc=0, in_adler=1, what=""):
    assert int(v["crc"][i]) == zlib.crc32(plain, in_crc), (what, i, len(plain))
    assert int(v["adler"][i]) == zlib.adler32(plain, in_adler), (what, i, len(plain))


def wrap(plain, deflate, fmt):
    if fmt == F.FMT_ZLIB:
        return b"\x78\x9c" + deflate + struct.pack(">I", zlib.adler32(plain))
    return F.gzip_header() + deflate + struct.pack("<II", zlib.crc32(plain), len(plain) & 0xffffffff)


def whole_streams():
    """-> [(fmt 0 raw / 1 zlib / 2 gzip, stream, plain)]: every kind at every size, the formats and levels in turn; level 0 of
    200 000 random bytes (stored runs of 65 535, longer than the ring); Z_FIXED; the fine index's and the build call's streams"""
    out, k = [], 0
    levels = [(1, zlib.Z_DEFAULT_STRATEGY), (6, zlib.Z_DEFAULT_STRATEGY), (9, zlib.Z_DEFAULT_STRATEGY), (6, zlib.Z_FIXED), (0, zlib.Z_DEFAULT_STRATEGY)]
    for n in SIZES:
        for kind in KINDS:
            d = make_block(kind, n, seed=k)
            lv, st = levels[k % len(levels)]
            fmt = k % 3
            out.append((fmt, raw(d, lv, st) if fmt == 0 else wrap(d, raw(d, lv, st), fmt), d))
            k += 1
    rnd = make_block("random", 200000, seed=99)
    for fmt in (0, 1, 2):
        out.append((fmt, raw(rnd, 0) if fmt == 0 else wrap(rnd, raw(rnd, 0), fmt), rnd))
        d = make_block("alice", 70000, seed=fmt)
        out.append((fmt, raw(d, 6, zlib.Z_FIXED) if fmt == 0 else wrap(d, raw(d, 6, zlib.Z_FIXED), fmt), d))
    for name, fmt, stream, plain in list(M.streams()) + list(B.streams()):
        if plain is not None:
            out.append((fmt, stream, plain))
    return out


@pytest.fixture(scope="module")
def whole():
    w = whole_streams()
    assert len(w) >= 8 * len(SIZES) + 6 + 11 and {f for f, _, _ in w} == {0, 1, 2}
    return w


def framed_both(eng, streams, caps, fmt, d=None):
    """verify_framed with dst = NULL beside decompress_framed[_dict] into real targets, sources at offsets (3 i) % 16:
    (verify results, verify frames, decode results, decode frames)"""
    n = len(streams)
    src, addrs = place(eng, streams, offs=[(3 * i) % 16 for i in range(n)])
    before = src.clone()
    hj = make_jobs(addrs, [len(s) for s in streams])
    wr, res = guarded(eng, n, pkg.RESULT_DTYPE)
    wf, frs = guarded(eng, n, pkg.FRAME_DTYPE)
    vres, vfr = eng.decompress_verify_framed(fmt, eng.to_device(hj), n, d, res, frs)
    v, vf = eng.results_to_host(vres).copy(), eng.frames_to_host(vfr).copy()
    assert guards_intact(wr) and guards_intact(wf) and bool((src == before).all())
    keep, tj = targets(eng, hj, caps)
    dj = eng.to_device(tj)
    dres, dfr = eng.decompress_framed_dict(fmt, d, dj, n) if d is not None else eng.decompress_framed(fmt, dj, n)
    return v, vf, eng.results_to_host(dres), eng.frames_to_host(dfr)


def same_as_the_decode(v, vf, r, f, i, what=""):
    for k in pkg.FRAME_DTYPE.names:
        assert int(vf[k][i]) == int(f[k][i]), (what, i, k, int(vf[k][i]), int(f[k][i]))
    assert int(v["cc"][i]) == int(r["cc"][i]), (what, i, int(v["cc"][i]), int(r["cc"][i]))
    if int(r["cc"][i]) in (0, 3) or int(f["status"][i]) not in (F.OK, F.TRUNCATED, F.DEFLATE, F.BAD_CHECK, F.BAD_LENGTH):
        for k in pkg.RESULT_DTYPE.names:                   # (a header failure: the refused record, in both)
            assert int(v[k][i]) == int(r[k][i]), (what, i, k, int(v[k][i]), int(r[k][i]))


# ---- whole streams ---------------------------------------------------------------------------------------------------------------
def test_whole_raw_streams_have_zlibs_checksums_and_the_size_calls_record(eng, whole):
    cases = [(s, p) for fmt, s, p in whole if fmt == 0]
    assert len(cases) >= 40
    v, s = run_raw(eng, [c for c, _ in cases], offs=[(3 * i) % 16 for i in range(len(cases))])
    for i, (c, p) in enumerate(cases):
        assert int(v["cc"][i]) == 0 and int(v["tpbc"][i]) == len(p), (i, len(p))
        same_record(v, s, i)
        sums_are(v, i, p)
        assert int(s["crc"][i]) == 0 and int(s["adler"][i]) == 0


def test_seeds_are_continued(eng, whole):
    cases = [(s, p) for fmt, s, p in whole if fmt == 0][::3]
    n = len(cases)
    rnd = random.Random(5)
    crcs = np.array([rnd.randrange(1 << 32) for _ in range(n)], np.uint32)
    adls = np.array([(rnd.randrange(65521) << 16) | rnd.randrange(65521) for _ in range(n)], np.uint32)
    v, s = run_raw(eng, [c for c, _ in cases], in_crc=crcs, in_adler=adls)
    for i, (c, p) in enumerate(cases):
        same_record(v, s, i)
        sums_are(v, i, p, int(crcs[i]), int(adls[i]))


def test_whole_framed_streams_equal_the_decode_into_real_targets(eng, whole):
    cases = [(s, p) for fmt, s, p in whole if fmt != 0]
    assert len(cases) >= 80
    v, vf, r, f = framed_both(eng, [c for c, _ in cases], [len(p) for _, p in cases], pkg.FMT_AUTO)
    for i, (c, p) in enumerate(cases):
        assert int(vf["status"][i]) == F.OK and int(v["cc"][i]) == 0 and int(v["tpbc"][i]) == len(p), (i, len(p))
        sums_are(v, i, p)
        same_as_the_decode(v, vf, r, f, i)
        assert int(vf["end"][i]) == len(c), i


# ---- damage the size call cannot see ---------------------------------------------------------------------------------------------
def framed_cases(dictionary):
    """tests/test_gpu_size.py's list: (family, stream, status of the SIZE call without a dictionary, with `dictionary`, plain or None)"""
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
    cmf = (z[0] & 0xf0) | 7                                                  # CM != 8 with a right FCHECK
    flg = z[1] & 0xe0
    flg += 31 - (cmf * 256 + flg) % 31
    return [
        ("z", z, F.OK, F.OK, plain), ("g", g, F.OK, F.OK, plain), ("g", g0, F.OK, F.OK, plain),
        ("z", flip(z, 1), F.BAD_HEADER, F.BAD_HEADER, None),                 # FCHECK
        ("z", bytes([cmf, flg]) + z[2:], F.BAD_METHOD, F.BAD_METHOD, None),
        ("g", g[:2] + b"\x07" + g[3:], F.BAD_METHOD, F.BAD_METHOD, None),
        ("z", zd, F.NEED_DICT, F.OK, dplain), ("z", zo, F.NEED_DICT, F.NEED_DICT, None),
        ("g", flip(g, ghl - 1), F.BAD_HCRC, F.BAD_HCRC, None),
        ("z", z[:1], F.TRUNCATED, F.TRUNCATED, None), ("g", g[:ghl - 3], F.TRUNCATED, F.TRUNCATED, None),     # inside the header
        ("z", z[:len(z) // 2], F.TRUNCATED, F.TRUNCATED, None), ("g", g[:len(g) // 2], F.TRUNCATED, F.TRUNCATED, None),   # the data
        ("z", z[:-2], F.TRUNCATED, F.TRUNCATED, None), ("g", g[:-5], F.TRUNCATED, F.TRUNCATED, None),         # the trailer
        ("z", bad_deflate_z, F.DEFLATE, F.DEFLATE, None), ("g", bad_deflate_g, F.DEFLATE, F.DEFLATE, None),
        ("g", flip(g, len(g) - 2), F.BAD_LENGTH, F.BAD_LENGTH, None),       # ISIZE
        ("z", flip(z, len(z) - 3), F.OK, F.OK, plain), ("g", flip(g, len(g) - 7, 0x80), F.OK, F.OK, plain),   # Adler-32 / CRC-32
        ("z", z + b"trailing", F.OK, F.OK, plain), ("g", g + g, F.OK, F.OK, plain),
    ]


ADLER_FLIP, CRC_FLIP = 18, 19                              # the two trailer flips in framed_cases


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


def fixed_block(literals, matches_every=0):
    w = FixedBits()
    for k, b in enumerate(literals):
        w.sym(b)
        if matches_every and k and k % matches_every == 0:
            w.match(9, 5)
    return w.done()


def test_trailer_flips_are_bad_check_where_the_size_call_says_ok(eng):
    dictionary = make_block("alice", 40000, seed=9)
    cases = framed_cases(dictionary)
    streams = [c[1] for c in cases]
    n = len(streams)
    v, vf, r, f = framed_both(eng, streams, [70000] * n, pkg.FMT_AUTO)
    src, addrs = place(eng, streams)
    sres, sfr = eng.decompress_size_framed(pkg.FMT_AUTO, eng.to_device(make_jobs(addrs, [len(s) for s in streams])), n)
    sf, sr = eng.frames_to_host(sfr), eng.results_to_host(sres)
    for i in (ADLER_FLIP, CRC_FLIP):
        assert int(vf["status"][i]) == F.BAD_CHECK and int(sf["status"][i]) == F.OK, i
        assert int(v["tpbc"][i]) == len(cases[i][4]) == int(sr["tpbc"][i])
        sums_are(v, i, cases[i][4])
    for i in range(n):                                     # everywhere else the two calls agree on the status
        if i not in (ADLER_FLIP, CRC_FLIP):
            assert int(vf["status"][i]) == int(sf["status"][i]) == cases[i][2], i


def test_damaged_payloads_and_isize(eng):
    rnd = make_block("random", 3000, seed=2)
    st = F.zlib_stream(rnd, 0)                             # one stored block: 2 + 5 bytes in front of the payload
    assert st[7:7 + 3000] == rnd
    st_bad = st[:1500] + bytes([st[1500] ^ 0x10]) + st[1501:]
    lits = [65 + (k * 7) % 60 for k in range(500)]
    twin = list(lits)
    twin[250] ^= 1                                         # (both below 144: the same 8 bits)
    good, bad = fixed_block(lits, 40), fixed_block(twin, 40)
    plain = zlib.decompressobj(-15).decompress(good)
    assert len(good) == len(bad) and len(zlib.decompressobj(-15).decompress(bad)) == len(plain) and plain[:500] != bytes(lits)
    fx, fx_bad = wrap(plain, good, F.FMT_GZIP), wrap(plain, bad, F.FMT_GZIP)
    g = F.gzip_member(make_block("alice", 20000, seed=5), 6)
    flip = lambda b, i, m=1: b[:i] + bytes([b[i] ^ m]) + b[i + 1:]
    streams = [st, st_bad, fx, fx_bad, flip(g, len(g) - 2), flip(flip(g, len(g) - 2), len(g) - 7, 0x80)]
    v, vf, r, f = framed_both(eng, streams, [30000] * len(streams), pkg.FMT_AUTO)
    assert [int(x) for x in vf["status"][:4]] == [F.OK, F.BAD_CHECK, F.OK, F.BAD_CHECK]
    assert int(v["tpbc"][1]) == int(v["tpbc"][0]) == 3000 and int(v["tpbc"][3]) == int(v["tpbc"][2]) == len(plain)
    sums_are(v, 0, rnd); sums_are(v, 2, plain)
    sums_are(v, 1, rnd[:1493] + bytes([rnd[1493] ^ 0x10]) + rnd[1494:])
    sums_are(v, 3, zlib.decompressobj(-15).decompress(bad))
    assert int(f["status"][4]) == F.BAD_LENGTH and int(f["status"][5]) in (F.BAD_CHECK, F.BAD_LENGTH)
    for i in range(len(streams)):                          # ISIZE, and ISIZE + CRC-32: whatever the decode reports
        same_as_the_decode(v, vf, r, f, i)


def test_the_framed_cases_equal_the_decode_with_and_without_the_dictionary(eng):
    dictionary = make_block("alice", 40000, seed=9)
    d = eng.dict_create(dictionary)
    try:
        cases = framed_cases(dictionary)
        for with_dict in (False, True):
            for fmt, fam in ((pkg.FMT_AUTO, "zg"), (pkg.FMT_ZLIB, "z"), (pkg.FMT_GZIP, "g")):
                pick = [c for c in cases if c[0] in fam]
                v, vf, r, f = framed_both(eng, [c[1] for c in pick], [70000] * len(pick), fmt, d if with_dict else None)
                seen = set()
                for i, c in enumerate(pick):
                    same_as_the_decode(v, vf, r, f, i, (fmt, with_dict))
                    seen.add(int(vf["status"][i]))
                    if int(vf["status"][i]) in (F.OK, F.BAD_CHECK) and c[4] is not None:
                        sums_are(v, i, c[4], what=(fmt, with_dict))
                if fmt == pkg.FMT_AUTO:
                    assert seen == {F.OK, F.BAD_HEADER, F.BAD_METHOD, F.NEED_DICT, F.BAD_HCRC, F.TRUNCATED, F.DEFLATE, F.BAD_CHECK, F.BAD_LENGTH}
                    assert int(vf["status"][6]) == (F.OK if with_dict else F.NEED_DICT)        # the FDICT job
                    assert int(vf["end"][20]) == len(cases[20][1]) - 8 and int(vf["end"][21]) == len(cases[21][1]) // 2   # trailing bytes, g + g
    finally:
        eng.torch.cuda.synchronize(eng.dev)
        d.close()


# ---- windows ---------------------------------------------------------------------------------------------------------------------
def test_a_window_in_front_of_the_stream_equals_the_decode(eng):
    import torch
    text = make_block("alice", 40000, seed=9)
    plain = make_block("alice", 20000, seed=5)
    bufs, hists, plains = [], [], []
    for h in (16, 4096, 32768):
        window = text[-h:]
        dplain = window[-3000:] + plain[:2000] + window[:1500] + plain[2000:2000 + 40000 // 2]     # reaches into the window at once
        bufs.append(window + raw(dplain, 6, zdict=window)); hists.append(h); plains.append(dplain)
    # a distance that ends at the window's first byte, and one a byte in front of it
    for h in (16, 32768):
        for dist in (h, h + 1):
            if dist <= 32768:
                w = FixedBits()
                w.match(7, dist)
                bufs.append(bytes(range(7, 7 + 16)) * (h // 16) + w.done()); hists.append(h); plains.append(None)
    n = len(bufs)
    v, s = run_raw(eng, bufs, offs=[(3 * i) % 16 for i in range(n)], hist=np.array(hists, np.uint32))
    src, addrs = place(eng, bufs)
    keep, tj = targets(eng, make_jobs(addrs, [len(b) for b in bufs], hist=np.array(hists, np.uint32)), [70000] * n)
    r = eng.results_to_host(eng.decompress(eng.to_device(tj), n))
    ccs = []
    for i in range(n):
        assert int(v["cc"][i]) == int(r["cc"][i]), (i, int(v["cc"][i]), int(r["cc"][i]))
        ccs.append(int(v["cc"][i]))
        same_record(v, s, i)
        if ccs[-1] == 0:
            for k in pkg.RESULT_DTYPE.names:
                assert int(v[k][i]) == int(r[k][i]), (i, k)
        if plains[i] is not None:
            assert ccs[-1] == 0
            sums_are(v, i, plains[i])
    assert ccs == [0, 0, 0, 0, 67, 0]
    h = bytes(range(7, 7 + 16))
    assert int(v["crc"][3]) == zlib.crc32(h[:7]) and int(v["crc"][5]) == zlib.crc32(h[:7])        # the window's first bytes, copied


def test_the_dictionary_is_the_window_of_the_jobs_that_name_it_and_of_no_other(eng):
    dictionary = make_block("alice", 40000, seed=9)
    plain = make_block("alice", 20000, seed=5)
    dplain = dictionary[-3000:] + plain[:2000] + dictionary[:1500]
    co = zlib.compressobj(6, zlib.DEFLATED, 15, 8, zlib.Z_DEFAULT_STRATEGY, dictionary)
    zd = co.compress(dplain) + co.flush()
    assert zd[1] & 0x20
    nodict = b"\x78\x9c" + zd[6:]                          # the same deflate data without FDICT: NXZ_JOB_NO_DICT, the distances reach nothing
    d = eng.dict_create(dictionary)
    try:
        v, vf, r, f = framed_both(eng, [zd, nodict, F.zlib_stream(plain)], [70000] * 3, pkg.FMT_ZLIB, d)
        assert [int(x) for x in vf["status"]] == [F.OK, F.DEFLATE, F.OK] and int(v["cc"][1]) == 67
        sums_are(v, 0, dplain); sums_are(v, 2, plain)
        for i in range(3):
            same_as_the_decode(v, vf, r, f, i)
    finally:
        eng.torch.cuda.synchronize(eng.dev)
        d.close()


# ---- early ends and the cap ------------------------------------------------------------------------------------------------------
def test_streams_cut_short_suspend_as_the_size_call_says_with_the_oracles_checksums(eng):
    rnd = random.Random(3)
    data = [(make_block("random", 70000, seed=1), 0, zlib.Z_DEFAULT_STRATEGY), (make_block("alice", 70000, seed=2), 6, zlib.Z_FIXED),
            (make_block("alice", 70000, seed=3), 6, zlib.Z_DEFAULT_STRATEGY), (make_block("lz", 70000, seed=4), 9, zlib.Z_DEFAULT_STRATEGY),
            (make_block("zeros", 70000, seed=5), 6, zlib.Z_DEFAULT_STRATEGY)]
    cases = []
    for d, lv, strat in data:
        c = raw(d, lv, strat)
        cuts = [0, 1, 2, 4, 5, 40, len(c) // 3, len(c) // 2, len(c) - 1] + [rnd.randrange(len(c)) for _ in range(4)]
        if lv == 0:
            cuts += [65535 + 5 + 3, 65535 + 5 + 5 + 100]   # inside the second stored block's header, inside its run
        cases += [c[:k] for k in cuts]
    v, s = run_raw(eng, cases, offs=[(3 * i) % 16 for i in range(len(cases))])
    kinds = set()
    for i, c in enumerate(cases):
        out, st = O.inflate(c, 80000)
        assert not st.err and int(v["cc"][i]) == 3 and int(v["tpbc"][i]) == len(out), (i, len(c))
        same_record(v, s, i)
        sums_are(v, i, out)
        kinds.add(int(v["sfbt"][i]) & 0xe)
    assert kinds == {0x8, 0xa, 0xc, 0xe}                   # inside stored, fixed and dynamic blocks, and in headers


def test_the_cap_and_the_jobs_it_refuses(eng, whole):
    by_size = {}
    for fmt, s, p in whole:
        if fmt == 0 and len(p) in (1, 65, PASS - 1, PASS, PASS + 1, 32769, 65536, 200000):
            by_size.setdefault(len(p), []).append((s, p))
    pick = [x for v_ in by_size.values() for x in v_[:2]]
    assert len(by_size) == 8 and len(pick) >= 12
    bufs, caps, plains = [], [], []
    for c, p in pick:
        for cap in (0, 1, len(p) - 1, len(p)):
            bufs.append(c); caps.append(cap); plains.append(p)
    v, s = run_raw(eng, bufs, caps=np.array(caps, np.uint32))
    for i, (cap, p) in enumerate(zip(caps, plains)):
        same_record(v, s, i)
        assert int(v["cc"][i]) == (0 if cap >= len(p) else 13), (i, cap, len(p))
        if cap >= len(p):
            sums_are(v, i, p)
    c = raw(b"hello hello hello")
    v, s = run_raw(eng, [c, c, bytes(32784) + c, c], hist=np.array([0, 0, 32784, 0], np.uint32), resume=np.array([0, 1, 0, 0x00e80000], np.uint32))
    assert int(v["cc"][0]) == 0 and int(v["tpbc"][0]) == 17 and int(v["crc"][0]) == zlib.crc32(b"hello hello hello")
    for i in (1, 2, 3):
        assert v[i].tolist() == REFUSED and s[i].tolist() == REFUSED, i


# ---- batch shape -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pool(eng, whole):
    """raw jobs of every sort with what they must give: (device source, host jobs, expected crc / adler or None, the size call's records)"""
    rnd = random.Random(12)
    bufs, hists, caps, sums = [], [], [], []
    for c, p in [(s, p) for fmt, s, p in whole if fmt == 0][::2]:
        bufs.append(c); hists.append(0); caps.append(NO_LIMIT); sums.append(p)
        k = rnd.randrange(len(c) + 1)                       # ... cut short
        bufs.append(c[:k]); hists.append(0); caps.append(NO_LIMIT); sums.append(O.inflate(c[:k], 210000)[0])
        bufs.append(c); hists.append(0); caps.append(len(p) // 2); sums.append(None if len(p) // 2 < len(p) else p)      # ... and capped
    text = make_block("alice", 40000, seed=9)
    for h in (16, 4096, 32768):
        body = text[-h:][:3000] + make_block("lz", 30000, seed=h)
        bufs.append(text[-h:] + raw(body, 6, zdict=text[-h:])); hists.append(h); caps.append(NO_LIMIT); sums.append(body)
    src, addrs = place(eng, bufs, offs=[(3 * i) % 16 for i in range(len(bufs))])
    hj = make_jobs(addrs, [len(b) for b in bufs], caps=np.array(caps, np.uint32), hist=np.array(hists, np.uint32))
    s = eng.results_to_host(eng.decompress_size(eng.to_device(hj), len(bufs))).copy()
    return src, hj, sums, s


@pytest.mark.parametrize("n", [1, 127, 128, 129, 300])
def test_a_job_gives_the_same_record_in_every_batch(eng, pool, n):
    """the by-length order switches on at 128 jobs; every record is independent of its neighbours"""
    src, hj, sums, s = pool
    m = len(hj)
    idx = (np.arange(n) * 7 + n) % m
    whole_, res = guarded(eng, n, pkg.RESULT_DTYPE)
    v = eng.results_to_host(eng.decompress_verify(eng.to_device(hj[idx]), n, res))
    assert guards_intact(whole_)
    for i, k in enumerate(idx):
        assert int(v["cc"][i]) == int(s["cc"][k]), (n, i, k)
        if int(s["cc"][k]) in (0, 3):
            for f in RECORD:
                assert int(v[f][i]) == int(s[f][k]), (n, i, k, f)
            assert sums[k] is not None
            sums_are(v, i, sums[k], what=(n, k))


def test_two_streams_at_once(eng, pool):
    L = eng.L
    L.nxz_stream_create.restype = C.c_void_p
    L.nxz_stream_create.argtypes = [C.c_void_p]
    L.nxz_stream_destroy.argtypes = [C.c_void_p, C.c_void_p]
    src, hj, sums, s = pool
    m, n = len(hj), 300                                    # (long streams first: the order workspace of each stream is in use)
    work = []
    for k in range(2):
        idx = (np.arange(n) * (3 + 2 * k) + k) % m
        work.append((eng.to_device(hj[idx]), eng.torch.empty(n * pkg.RESULT_DTYPE.itemsize, dtype=eng.torch.uint8, device=eng.dev), idx))
    eng.torch.cuda.synchronize(eng.dev)
    handles = [L.nxz_stream_create(eng.ctx) for _ in range(2)]
    assert all(handles)
    rcs = [None, None]

    def run(k):
        jobs, res, idx = work[k]
        rc = 0
        for _ in range(3):
            rc = rc or L.nxz_batch_decompress_verify(eng.ctx, jobs.data_ptr(), n, res.data_ptr(), C.c_void_p(handles[k]))
        rcs[k] = rc or L.nxz_ctx_sync(eng.ctx, C.c_void_p(handles[k]))
    threads = [threading.Thread(target=run, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert rcs == [0, 0]
    for k in range(2):
        jobs, res, idx = work[k]
        v = eng.results_to_host(res)
        for i, j in enumerate(idx):
            assert int(v["cc"][i]) == int(s["cc"][j]), (k, i)
            if int(s["cc"][j]) in (0, 3):
                assert int(v["tpbc"][i]) == int(s["tpbc"][j]), (k, i)
                sums_are(v, i, sums[j], what=(k, i))
    for h in handles:
        L.nxz_stream_destroy(eng.ctx, C.c_void_p(h))


# ---- arguments -------------------------------------------------------------------------------------------------------------------
def test_argument_checks(eng):
    import errno
    L = eng.L
    j, r = eng.torch.zeros(48, dtype=eng.torch.uint8, device=eng.dev), eng.torch.zeros(64, dtype=eng.torch.uint8, device=eng.dev)
    sh = eng.stream_handle()
    assert L.nxz_batch_decompress_verify(eng.ctx, None, 0, None, sh) == 0
    assert L.nxz_batch_decompress_verify_framed(eng.ctx, pkg.FMT_ZLIB, None, None, 0, None, None, sh) == 0
    assert L.nxz_batch_decompress_verify(None, j.data_ptr(), 1, r.data_ptr(), sh) == -errno.EINVAL
    assert L.nxz_batch_decompress_verify(eng.ctx, None, 1, r.data_ptr(), sh) == -errno.EINVAL
    assert L.nxz_batch_decompress_verify(eng.ctx, j.data_ptr(), 1, None, sh) == -errno.EINVAL
    assert L.nxz_batch_decompress_verify(eng.ctx, j.data_ptr(), 1 << 31, r.data_ptr(), sh) == -errno.EINVAL
    for fmt in (0, 4):                                     # (raw has no frame: the raw call; beyond FMT_AUTO)
        assert L.nxz_batch_decompress_verify_framed(eng.ctx, fmt, None, j.data_ptr(), 1, r.data_ptr(), r.data_ptr(), sh) == -errno.EINVAL
    assert L.nxz_batch_decompress_verify_framed(eng.ctx, pkg.FMT_ZLIB, None, j.data_ptr(), 1, r.data_ptr(), None, sh) == -errno.EINVAL
