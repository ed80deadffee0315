"""GPU tests of the device-side zlib / gzip framing (include/nxz_engine.h: nxz_batch_decompress_framed, nxz_batch_unpack_gzip,
nxz_batch_pack_zlib; kernels in power-gzip_amd/csrc/nxz_frame.hip): bytes against the plain data, frames[] against an
independent Python reading of the headers and trailers (tests/framing.py), results[] against nxz_batch_decompress on the same
streams with their framing cut off by hand, the statuses of damaged streams, and BGZF images of every origin."""
import ctypes as C
import errno
import importlib
import os
import random
import struct
import zlib

import numpy as np
import pytest

import framing as F
from datagen import make_block

pytestmark = pytest.mark.gpu
pkg = importlib.import_module("power-gzip_amd")
CC_INVALID_OP = 8
KNOBS = ("NXZ_INFLATE_LANES_MIN", "NXZ_INFLATE_CUT", "NXZ_INFLATE_WG", "NXZ_INFLATE_WG_MAX", "NXZ_WG_PMIN", "NXZ_INFLATE_ORDER")


@pytest.fixture(scope="module")
def eng():
    saved = {k: os.environ.pop(k, None) for k in KNOBS}
    e = pkg.Engine(0)
    yield e
    e.close()
    for k, v in saved.items():
        if v is not None:
            os.environ[k] = v


class Case:
    """one framed stream: hdr + body (raw deflate) + trailer + tail (bytes after the trailer)"""

    def __init__(self, plain, fmt, hdr, body, trailer, tail=b""):
        self.plain, self.fmt, self.hdr, self.body, self.trailer, self.tail = plain, fmt, hdr, body, trailer, tail

    @property
    def stream(self):
        return self.hdr + self.body + self.trailer + self.tail


def zcase(plain, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, wbits=15):
    s = F.zlib_stream(plain, level, strategy, wbits)
    return Case(plain, F.FMT_ZLIB, s[:2], s[2:-4], s[-4:])


def gcase(plain, level=6, **hdr):
    return Case(plain, F.FMT_GZIP, F.gzip_header(**hdr), F.raw_deflate(plain, level),
                struct.pack("<II", zlib.crc32(plain), len(plain) & 0xffffffff))


def _jobs(eng, bufs, offs, caps, sentinel=0xcd):
    """bufs placed at offs[i] into rows of one device tensor; outputs 16-byte aligned rows filled with `sentinel`"""
    import torch
    n = len(bufs)
    sstride = (max(len(b) + o for b, o in zip(bufs, offs)) + 16 + 15) & ~15
    host = np.full((n, sstride), 0xa5, np.uint8)
    for i, b in enumerate(bufs):
        host[i, offs[i]:offs[i] + len(b)] = np.frombuffer(b, np.uint8)
    src = torch.from_numpy(host).to(eng.dev)
    ostride = (max(caps) + 16 + 15) & ~15
    dst = torch.full((n, ostride), sentinel, dtype=torch.uint8, device=eng.dev)
    j = np.zeros(n, pkg.JOB_DTYPE)
    j["src"] = np.uint64(src.data_ptr()) + np.arange(n, dtype=np.uint64) * np.uint64(sstride) + np.array(offs, np.uint64)
    j["dst"] = np.uint64(dst.data_ptr()) + np.arange(n, dtype=np.uint64) * np.uint64(ostride)
    j["src_len"] = [len(b) for b in bufs]
    j["dst_cap"] = caps
    j["in_adler"] = 1
    return src, dst, eng.to_device(j)


def framed(eng, streams, fmt, caps, offs=None, sentinel=0xcd):
    offs = offs or [0] * len(streams)
    src, dst, jobs = _jobs(eng, streams, offs, caps, sentinel)
    res, fr = eng.decompress_framed(fmt, jobs, len(streams))
    return eng.results_to_host(res), eng.frames_to_host(fr), dst.cpu().numpy()


def raw(eng, bodies, caps):
    src, dst, jobs = _jobs(eng, bodies, [0] * len(bodies), caps)
    return eng.results_to_host(eng.decompress(jobs, len(bodies))), dst.cpu().numpy()


def expected_frame(c, fmt):
    want = F.parse(c.stream, fmt)
    assert want["status"] == F.OK and want["hdr_len"] == len(c.hdr)
    want["end"] = len(c.hdr) + len(c.body) + len(c.trailer)
    if c.fmt == F.FMT_ZLIB:
        want["check"], want["isize"] = struct.unpack(">I", c.trailer)[0], 0
    else:
        want["check"], want["isize"] = struct.unpack("<II", c.trailer)
    return want


def check_batch(eng, cases, fmt, offs=None, slack=0):
    caps = [len(c.plain) + slack for c in cases]
    r, f, out = framed(eng, [c.stream for c in cases], fmt, caps, offs)
    rr, _ = raw(eng, [c.body for c in cases], caps)
    for i, c in enumerate(cases):
        got = {k: int(f[k][i]) for k in list(F.FIELDS) + ["end", "check", "isize"]}
        assert got == expected_frame(c, fmt), i
        assert out[i, :len(c.plain)].tobytes() == c.plain, i
        assert r[i].tobytes() == rr[i].tobytes(), (i, r[i], rr[i])
    return r, f


def test_zlib_levels_strategies_sizes_offsets(eng):
    strategies = [zlib.Z_DEFAULT_STRATEGY, zlib.Z_FILTERED, zlib.Z_HUFFMAN_ONLY, zlib.Z_RLE, zlib.Z_FIXED]
    kinds = ["alice", "lz", "text33", "zeros", "random", "periodic", "binary", "sparse"]
    sizes = [0, 1, 17, 1000, 65536, 100000, 300000, 2 << 20]
    cases = []
    k = 0
    for level in range(10):
        for si, st in enumerate(strategies):
            n = sizes[(level + si) % len(sizes)]
            cases.append(zcase(make_block(kinds[k % len(kinds)], n, seed=k) if n else b"", level, st, wbits=9 + k % 7))
            k += 1
    check_batch(eng, cases, F.FMT_ZLIB, offs=[i % 16 for i in range(len(cases))])


def test_gzip_fields_and_auto(eng):
    rnd = random.Random(1)
    cases = []
    for flg in range(32):
        plain = make_block(["alice", "lz", "text33"][flg % 3], 1000 + 997 * flg, seed=flg)
        cases.append(gcase(plain, level=1 + flg % 9, flg=flg, mtime=rnd.getrandbits(32), xfl=flg, os_=3,
                           extra=b"XY\x02\x00ab" * (flg % 4), name=b"name-%d.txt" % flg * (1 + flg % 3),
                           comment=bytes(rnd.randrange(1, 256) for _ in range(100 + 1000 * (flg % 2)))))
    check_batch(eng, cases, F.FMT_GZIP, offs=[(3 * i) % 16 for i in range(len(cases))])
    # a mixed batch: the format per job
    mixed = [cases[i] if i % 2 else zcase(make_block("lz", 5000 + i, seed=i), i % 10) for i in range(24)]
    r, f = check_batch(eng, mixed, F.FMT_AUTO, offs=[i % 16 for i in range(24)])
    assert [int(x) for x in f["format"]] == [F.FMT_GZIP if i % 2 else F.FMT_ZLIB for i in range(24)]


def test_whole_valid_streams_stay_on_the_workgroup_route(eng):
    """4096 zlib streams of 64 KiB blocks, every knob unset: none goes back to the stream-per-wavefront kernel"""
    kinds = ["alice", "lz", "text33", "periodic", "binary", "sparse"]
    plains = [make_block(kinds[i % len(kinds)], 65536, seed=i % 64) for i in range(64)]
    streams = [zlib.compress(p, 6) for p in plains]
    n = 4096
    r, f, out = framed(eng, [streams[i % 64] for i in range(n)], F.FMT_ZLIB, [65536] * n, offs=[i % 16 for i in range(n)])
    assert (f["status"] == F.OK).all() and (r["cc"] == 0).all() and (r["tpbc"] == 65536).all()
    assert all(out[i, :65536].tobytes() == plains[i % 64] for i in range(0, n, 61))
    assert eng.wg_reasons()["handed_back"] == 0


def test_failures(eng):
    plain = make_block("alice", 20000, seed=5)
    z, g = zcase(plain), gcase(plain, flg=F.FNAME, name=b"a.txt")
    streams, want = [], []
    for b in range(4):                               # each trailer byte, one bit flipped
        t = bytearray(z.trailer); t[b] ^= 1 << b
        streams.append(z.hdr + z.body + bytes(t)); want.append(F.BAD_CHECK)
    for b in range(8):
        t = bytearray(g.trailer); t[b] ^= 0x80 >> b
        streams.append(g.hdr + g.body + bytes(t)); want.append(F.BAD_CHECK if b < 4 else F.BAD_LENGTH)
    for cut in range(1, 5):                          # a cut trailer
        streams.append(z.stream[:-cut]); want.append(F.TRUNCATED)
    for cut in (1, 4, 7, 8):
        streams.append(g.stream[:-cut]); want.append(F.TRUNCATED)
    streams.append(z.stream + b"trailing"); want.append(F.OK)
    streams.append(g.stream + g.stream); want.append(F.OK)
    damaged = bytes([z.body[0] | 6]) + z.body[1:]    # BTYPE 3
    streams.append(z.hdr + damaged + z.trailer); want.append(F.DEFLATE)
    streams.append(bytes([z.hdr[0], z.hdr[1] ^ 1]) + z.body + z.trailer); want.append(F.BAD_HEADER)
    streams.append(g.hdr[:5]); want.append(F.TRUNCATED)
    n = len(streams)
    r, f, out = framed(eng, streams, F.FMT_AUTO, [len(plain)] * n, offs=[i % 16 for i in range(n)], sentinel=0x5a)
    assert [int(s) for s in f["status"]] == want
    assert int(f["end"][n - 5]) == len(z.stream) and int(f["end"][n - 4]) == len(g.stream)
    for i in range(12):                              # checksums wrong: the trailer as read
        assert out[i, :len(plain)].tobytes() == plain and int(f["check"][i]) == struct.unpack(">I" if i < 4 else "<I", streams[i][-4 if i < 4 else -8:][:4])[0]
    rr, _ = raw(eng, [damaged], [len(plain)])
    assert r[n - 3].tobytes() == rr[0].tobytes() and int(r["cc"][n - 3]) not in (0, 3)
    for i in (n - 2, n - 1):                         # header failures: nothing decoded, dst untouched
        assert r[i].tolist() == (CC_INVALID_OP, 0, 0, 0, 0, 0, 0, 0)
        assert (out[i] == 0x5a).all()
    # FDICT: nothing decoded, the dictionary's id reported
    c = zlib.compressobj(6, zlib.DEFLATED, 15, 8, zlib.Z_DEFAULT_STRATEGY, zdict=b"some dictionary")
    fd = c.compress(plain) + c.flush()
    r, f, out = framed(eng, [fd], F.FMT_ZLIB, [len(plain)], sentinel=0x5a)
    assert int(f["status"][0]) == F.NEED_DICT and int(f["dictid"][0]) == zlib.adler32(b"some dictionary") and (out[0] == 0x5a).all()


# ---- BGZF images ---------------------------------------------------------------------------------------------------------
def unpack(eng, image, total, max_members=None, dst_cap=None):
    import torch
    pad = np.full(len(image) + 64, 0xee, np.uint8)
    pad[3:3 + len(image)] = np.frombuffer(image, np.uint8)            # (an image that does not start on a 16-byte boundary)
    t = torch.from_numpy(pad).to(eng.dev)
    packed = t[3:]
    dst = torch.full((dst_cap if dst_cap is not None else max(total, 1),), 0xcd, dtype=torch.uint8, device=eng.dev)
    mm = max_members if max_members is not None else len(image) // 26 + 1
    rc, d = eng.unpack_gzip(packed, len(image), dst, mm)
    torch.cuda.synchronize(eng.dev)
    return rc, d, dst


def check_image(eng, image, plains):
    total = sum(len(p) for p in plains)
    assert len(F.bgzf_scan(image)[0]) == len(plains)
    rc, d, dst = unpack(eng, image, total)
    assert rc == 0, rc
    assert d["members"] == len(plains) and d["out_len"] == total
    assert dst.cpu().numpy()[:total].tobytes() == b"".join(plains)
    m = d["members"]
    f = eng.frames_to_host(d["frames"])[:m]
    assert (f["status"] == F.OK).all() and (f["format"] == F.FMT_GZIP).all()
    offs = d["offsets"].cpu().numpy()[:m + 1]
    assert offs.tolist() == np.concatenate([[0], np.cumsum([len(p) for p in plains])]).tolist()
    return d


SINK = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t)


class BlockedOpts(C.Structure):
    """nxz_blocked_opts_t (include/nxz_blocked.h)"""
    _fields_ = [("device", C.c_int), ("fixed", C.c_int), ("block_size", C.c_uint32), ("chunk_blocks", C.c_uint32),
                ("group", C.c_uint32), ("reserved", C.c_uint32 * 3)]


def blocked_lib():
    L = C.CDLL(os.path.join(os.path.dirname(pkg.lib_path()), "libnxz_amd.so"))
    L.nxz_blocked_scan.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_size_t)]
    L.nxz_blocked_deflate.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(BlockedOpts), SINK, C.c_void_p, C.POINTER(C.c_uint64)]
    L.nxz_blocked_end_marker.argtypes = [SINK, C.c_void_p]
    return L


def blocked_image(data):
    """nxz_blocked_deflate's members of data, then the end marker"""
    parts = []

    def cb(user, buf, n):
        parts.append(C.string_at(buf, n))
        return 0
    sink = SINK(cb)
    L = blocked_lib()
    o = BlockedOpts(device=0)
    assert L.nxz_blocked_deflate(data, len(data), C.byref(o), sink, None, None) == 0
    assert L.nxz_blocked_end_marker(sink, None) == 0
    return b"".join(parts)


def test_unpack_images_of_every_origin(eng):
    import torch
    rnd = random.Random(9)
    data = b"".join(make_block(["alice", "lz", "text33", "random"][i % 4], 65280, seed=i) for i in range(24)) + b"tail" * 999
    # 1. nxz_blocked_deflate (libnxz_amd.so), with the end marker
    img = blocked_image(data)
    chunks = [data[i:i + 65280] for i in range(0, len(data), 65280)] + [b""]
    check_image(eng, img, chunks)
    # 2. nxz_batch_pack_gzip from a compress batch on the device, with the end marker
    n = len(chunks) - 1
    host = np.zeros((n, 65280), np.uint8)
    for i, ch in enumerate(chunks[:-1]):
        host[i, :len(ch)] = np.frombuffer(ch, np.uint8)
    src = torch.from_numpy(host).to(eng.dev)
    cdst = torch.zeros((n, 73856), dtype=torch.uint8, device=eng.dev)
    jobs = eng.jobs_strided(src, 65280, np.array([len(c) for c in chunks[:-1]], np.uint32), cdst, 73856, 73856)
    res, _ = eng.compress(pkg.FC_COMPRESS_DHTGEN, jobs, n)
    packed = torch.zeros(n * (65280 + 40) + 64, dtype=torch.uint8, device=eng.dev)
    offs = eng.pack_gzip(jobs, res, n, packed)
    torch.cuda.synchronize(eng.dev)
    img2 = packed.cpu().numpy()[:int(offs[n].item())].tobytes() + F.BGZF_EOF
    check_image(eng, img2, chunks)
    # 3. Python-built members with subfields before and after BC, odd sizes, and trailing foreign bytes
    plains = [make_block("alice", rnd.choice([7, 1000, 33333, 65280, 50001]), seed=i) for i in range(40)]
    img3 = b"".join(F.bgzf_member(p, before=b"XY" + struct.pack("<H", 4 * (i % 2)) + bytes(4) * (i % 2), after=b"Z\x01\x01\x00q" * (i % 3),
                                  mtime=i) for i, p in enumerate(plains))
    check_image(eng, img3, plains)
    tail = img3 + b"foreign bytes, not a member" * 5
    d = check_image(eng, tail, plains)
    consumed = C.c_size_t()
    assert blocked_lib().nxz_blocked_scan(tail, len(tail), None, None, C.byref(consumed)) == 0
    assert d["consumed"] == consumed.value == len(img3)


def test_unpack_false_member_inside_a_payload(eng):
    """a stored payload that holds a valid-looking member header whose size leads to the next true member"""
    fake = bytearray(F.bgzf_member(b"zz")[:18])
    first = b"q" * 100 + bytes(fake) + b"r" * 200
    a_len = 18 + 5 + len(first) + 8
    fake[16:18] = struct.pack("<H", a_len - (18 + 5 + 100) - 1)
    first = b"q" * 100 + bytes(fake) + b"r" * 200
    a = F.bgzf_member(first, level=0)
    assert len(a) == a_len and F.bgzf_member_size(a, 123) == a_len - 123
    plains = [first] + [make_block("lz", 3000 + i, seed=i) for i in range(5)]
    img = a + b"".join(F.bgzf_member(p) for p in plains[1:])
    d = check_image(eng, img, plains)
    assert d["members"] == 6 and d["consumed"] == len(img)


def test_unpack_many_small_members(eng):
    rnd = random.Random(2)
    words = [b"alpha", b"beta", b"gamma", b"delta", b"\x00\x01", b"1f8b"]
    plains = [b" ".join(rnd.choice(words) for _ in range(rnd.randrange(0, 12))) for _ in range(100000)]
    img = b"".join(F.bgzf_member(p, level=1 + i % 9) for i, p in enumerate(plains)) + F.BGZF_EOF
    d = check_image(eng, img, plains + [b""])
    assert d["members"] == 100001 and d["consumed"] == len(img)


def test_unpack_errors(eng):
    plains = [make_block("text33", 4000 + i, seed=i) for i in range(10)]
    img = b"".join(F.bgzf_member(p) for p in plains)
    total = sum(len(p) for p in plains)
    rc, d, _ = unpack(eng, img, total, max_members=9)
    assert rc == -errno.E2BIG and d["members"] == 10
    rc, d, _ = unpack(eng, img, total, dst_cap=total - 1)
    assert rc == -errno.E2BIG and d["out_len"] == total
    rc, d, _ = unpack(eng, b"x" + img, total)
    assert rc == -errno.EILSEQ


def test_pack_zlib_round_trip(eng):
    import torch
    blocks = [make_block(k, n, seed=i) for i, (k, n) in enumerate([("alice", 65280), ("random", 5000), ("zeros", 4096), ("lz", 30000),
                                                                     ("text33", 17), ("random", 65280), ("binary", 40000)])]
    n = len(blocks)
    host = np.zeros((n, 65280), np.uint8)
    for i, b in enumerate(blocks):
        host[i, :len(b)] = np.frombuffer(b, np.uint8)
    src = torch.from_numpy(host).to(eng.dev)
    cdst = torch.zeros((n, 73856), dtype=torch.uint8, device=eng.dev)
    jobs = eng.jobs_strided(src, 65280, np.array([len(b) for b in blocks], np.uint32), cdst, 73856, 73856)
    res, _ = eng.compress(pkg.FC_COMPRESS_DHTGEN, jobs, n)
    for level in (-1, 0, 1, 5, 9):
        packed = torch.zeros(n * (65280 + 16) + 64, dtype=torch.uint8, device=eng.dev)
        offs = eng.pack_zlib(level, jobs, res, n, packed)
        torch.cuda.synchronize(eng.dev)
        o = offs.cpu().numpy()
        pk = packed.cpu().numpy()
        members = [pk[o[i]:o[i + 1]].tobytes() for i in range(n)]
        flevel = {-1: 2, 0: 0, 1: 0, 5: 1, 9: 3}[level]
        for b, m in zip(blocks, members):
            assert zlib.decompress(m) == b and m[0] == 0x78 and m[1] >> 6 == flevel
        # and back through the framed path, straight from the packed image (sources at any alignment)
        j = np.zeros(n, pkg.JOB_DTYPE)
        out = torch.full((n, 65536), 0xcd, dtype=torch.uint8, device=eng.dev)
        j["src"] = np.uint64(packed.data_ptr()) + o[:n].astype(np.uint64)
        j["src_len"] = np.diff(o)
        j["dst"] = np.uint64(out.data_ptr()) + np.arange(n, dtype=np.uint64) * np.uint64(65536)
        j["dst_cap"] = 65536
        r, fr = eng.decompress_framed(pkg.FMT_ZLIB, eng.to_device(j), n)
        f = eng.frames_to_host(fr)
        got = out.cpu().numpy()
        assert (f["status"] == F.OK).all() and (f["end"] == np.diff(o)).all()
        for i, b in enumerate(blocks):
            assert got[i, :len(b)].tobytes() == b
