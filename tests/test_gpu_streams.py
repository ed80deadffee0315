"""GPU tests of nxz_batch_deflate_streams (include/nxz_engine.h; the kernels in power-gzip_amd/csrc/nxz_streams.hip): a batch of
device buffers of any length, each written as one raw, zlib or gzip stream.  The yardsticks are zlib (every stream decompresses to
its source, the checksums are zlib's) and nxz_deflate_host_hist, the engine's own host-buffer path, whose raw stream the deflate
data must equal byte for byte; the framing is spelled out here."""
import ctypes as C
import errno
import importlib
import os
import struct
import zlib

import numpy as np
import pytest

from datagen import make_block

pytestmark = pytest.mark.gpu
pkg = importlib.import_module("power-gzip_amd")
RAW, ZLIB, GZIP = pkg.engine.FMT_RAW, pkg.engine.FMT_ZLIB, pkg.engine.FMT_GZIP
SJ, SR = pkg.engine.STREAM_JOB_DTYPE, pkg.engine.STREAM_RESULT_DTYPE
FHT, DHTGEN, DHT = pkg.FC_COMPRESS_FHT, pkg.FC_COMPRESS_DHTGEN, pkg.FC_COMPRESS_DHT
WBITS = {RAW: -15, ZLIB: 15, GZIP: 31}
CANARY, TAIL = 0xc3, 64
GZIP_HEADER = bytes.fromhex("1f8b0800000000000403")
ZLIB_HEADER = {-1: b"\x78\x9c", 1: b"\x78\x01", 5: b"\x78\x5e", 6: b"\x78\x9c", 9: b"\x78\xda"}


@pytest.fixture(scope="module")
def eng():
    e = pkg.Engine(0)
    e.L.nxz_deflate_host_bound_hist.restype = C.c_size_t
    e.L.nxz_deflate_host_bound_hist.argtypes = [C.c_size_t, C.c_uint32]
    e.L.nxz_deflate_host_hist.argtypes = [C.c_void_p, C.c_int, C.c_char_p, C.c_size_t, C.c_int, C.c_uint32, C.c_char_p, C.c_size_t,
                                          C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    yield e
    e.close()


def block_bytes(hist_max):
    return 65536 - min(hist_max & ~15, 32768)


_mixed = {}


def mixed(n, seed):
    """n bytes, 64 KiB pieces of the four kinds in turn (made once per size)"""
    if (n, seed) not in _mixed:
        kinds, out, k = ["alice", "lz", "zeros", "random"], [], 0
        while sum(len(p) for p in out) < n:
            out.append(make_block(kinds[(k + seed) % 4], min(65536, n - 65536 * k), seed=seed + k))
            k += 1
        _mixed[(n, seed)] = b"".join(out)
    return _mixed[(n, seed)]


def edge_buffers(hist_max):
    B = block_bytes(hist_max)
    return [b"", make_block("alice", 1, 1), make_block("lz", 15, 2), make_block("zeros", 16, 3), make_block("alice", B - 1, 4),
            make_block("random", B, 5), make_block("lz", B + 1, 6), mixed(2 * B, 7), mixed(2 * B + 17, 8), mixed(65 * B + 5, 9)]


_ref = {}


def host_stream(eng, fc, data, hist_max):
    """the raw deflate stream nxz_deflate_host_hist writes for `data` (final, no earlier input) -- the parent's code"""
    key = (fc, hist_max, hash(data), len(data))
    if key not in _ref:
        if not data:
            _ref[key] = bytes.fromhex("010000ffff")          # (the host call takes no empty buffer; tests/test_stream.py has these bytes)
        else:
            cap = eng.L.nxz_deflate_host_bound_hist(len(data), hist_max)
            dst = C.create_string_buffer(cap)
            n, crc, adler = C.c_size_t(), C.c_uint32(), C.c_uint32()
            rc = eng.L.nxz_deflate_host_hist(eng.ctx, fc, data, len(data), 1, hist_max, None, 0, dst, cap, C.byref(n), C.byref(crc), C.byref(adler))
            assert rc == 0 and crc.value == zlib.crc32(data) and adler.value == zlib.adler32(data)
            _ref[key] = dst.raw[:n.value]
    return _ref[key]


def framed(fmt, level, body, data):
    if fmt == ZLIB:
        return ZLIB_HEADER[level] + body + struct.pack(">I", zlib.adler32(data))
    if fmt == GZIP:
        return GZIP_HEADER + body + struct.pack("<II", zlib.crc32(data), len(data) & 0xffffffff)
    return body


class Run:
    """one call: sources at 16-byte aligned offsets of one device buffer, targets in slots of one device buffer filled with canary bytes"""

    def __init__(self, eng, fc, fmt, bufs, hist_max=0, level=-1, dst_off=None, cap_delta=None, src_off=None, null_dst=()):
        import torch
        n = len(bufs)
        dst_off = dst_off or [0] * n
        cap_delta = cap_delta or [0] * n
        src_off = src_off or [0] * n
        self.bound = [eng.deflate_stream_bound(len(b), hist_max, fmt) for b in bufs]
        self.cap = [b + d for b, d in zip(self.bound, cap_delta)]
        sat, pos = [], 0
        for b, o in zip(bufs, src_off):
            sat.append(pos + o)
            pos += (o + len(b) + 31) & ~15
        hs = np.zeros(pos + 16, np.uint8)
        for b, a in zip(bufs, sat):
            hs[a:a + len(b)] = np.frombuffer(b, np.uint8)
        self.dat, pos = [], 0
        for c, o in zip(self.cap, dst_off):
            self.dat.append(pos + 16 + o)
            pos += (16 + o + c + TAIL + 15) & ~15
        self.src = torch.from_numpy(hs).to(eng.dev)
        self.dst = torch.full((pos + 16,), CANARY, dtype=torch.uint8, device=eng.dev)
        j = np.zeros(n, SJ)
        for i in range(n):
            j[i] = (self.src.data_ptr() + sat[i], 0 if i in null_dst else self.dst.data_ptr() + self.dat[i], len(bufs[i]), self.cap[i])
        self.jobs = j
        self.rc, res = eng.deflate_stream_jobs(fc, fmt, j, hist_max=hist_max, level=level)
        j[:] = 0                                               # (the array may be reused as soon as the call returns)
        self.res = eng.results_to_host(res, SR)[:n].copy()
        self.out = self.dst.cpu().numpy()
        self.slot_end = [a + c + TAIL for a, c in zip(self.dat, self.cap)]

    def stream(self, i):
        return self.out[self.dat[i]:self.dat[i] + int(self.res["out_len"][i])].tobytes()

    def untouched(self, i, used):
        """everything of slot i but its first `used` bytes still holds the canary"""
        lo = self.slot_end[i - 1] if i else 0
        return bool((self.out[lo:self.dat[i]] == CANARY).all() and (self.out[self.dat[i] + used:self.slot_end[i]] == CANARY).all())


def check_stream(run, i, fmt, data, B):
    r = run.res[i]
    assert r["cc"] == 0, (i, r)
    s = run.stream(i)
    d = zlib.decompressobj(WBITS[fmt])
    assert d.decompress(s) == data and d.eof and d.unused_data == b"", i
    assert r["crc"] == zlib.crc32(data) and r["adler"] == zlib.adler32(data), (i, r)
    assert r["blocks"] == (len(data) + B - 1) // B and r["out_len"] <= run.bound[i], (i, r)
    assert run.untouched(i, int(r["out_len"])), i
    return s


@pytest.mark.parametrize("fc", [FHT, DHTGEN])
@pytest.mark.parametrize("hist_max", [0, 4096, 32768])
def test_edges_of_the_cut(eng, fc, hist_max):
    B = block_bytes(hist_max)
    bufs = edge_buffers(hist_max)
    assert [len(b) for b in bufs] == [0, 1, 15, 16, B - 1, B, B + 1, 2 * B, 2 * B + 17, 65 * B + 5]
    for i, b in enumerate(bufs):
        assert eng.deflate_stream_bound(len(b), hist_max, RAW) == eng.L.nxz_deflate_host_bound_hist(len(b), hist_max)
        assert eng.deflate_stream_bound(len(b), hist_max, ZLIB) == eng.deflate_stream_bound(len(b), hist_max, RAW) + 6
        assert eng.deflate_stream_bound(len(b), hist_max, GZIP) == eng.deflate_stream_bound(len(b), hist_max, RAW) + 18
    raws = None
    for fmt, level in ((RAW, -1), (ZLIB, 5), (GZIP, -1)):
        run = Run(eng, fc, fmt, bufs, hist_max, level)
        assert run.rc == 0
        got = [check_stream(run, i, fmt, b, B) for i, b in enumerate(bufs)]
        if fmt == RAW:
            raws = got
            for i, b in enumerate(bufs):
                assert got[i] == host_stream(eng, fc, b, hist_max), "stream %d is not nxz_deflate_host_hist's" % i
            if hist_max == 0:
                # random bytes do not shrink: one stored block of 65536 bytes, which takes two headers
                assert run.res["stored"][5] == 1 and got[5][:5] == bytes.fromhex("00ffff0000") and len(got[5]) == 65536 + 10
                assert got[5][5 + 65535:5 + 65535 + 5] == bytes.fromhex("0101 00fe ff".replace(" ", ""))
            assert run.res["stored"][0] == 0 and run.res["stored"][9] >= 1
        else:
            for i, b in enumerate(bufs):
                assert got[i] == framed(fmt, level, raws[i], b), (fmt, i)


def test_chunks_do_not_show(eng, monkeypatch):
    hist_max = 32768
    bufs = edge_buffers(hist_max) + [make_block("alice", 3000 + 17 * k, 20 + k) for k in range(10)]
    monkeypatch.delenv("NXZ_STREAMS_CHUNK", raising=False)
    base = Run(eng, DHTGEN, GZIP, bufs, hist_max)
    assert base.rc == 0 and (base.res["cc"] == 0).all() and base.res["blocks"].sum() == 78 + 10
    for chunk in (1, 3, 64):
        monkeypatch.setenv("NXZ_STREAMS_CHUNK", str(chunk))
        run = Run(eng, DHTGEN, GZIP, bufs, hist_max)
        assert run.rc == 0
        assert run.res.tobytes() == base.res.tobytes(), chunk
        assert np.array_equal(run.out, base.out), chunk


def test_many_small_streams(eng):
    import torch
    n, stride, dstride = 66000, 64, 96
    rnd = np.random.default_rng(11)
    lens = rnd.integers(16, 49, n)
    hs = rnd.integers(97, 101, (n, stride), dtype=np.uint8)
    hs[:, 0:4] = np.arange(n, dtype="<u4").view(np.uint8).reshape(n, 4)       # every stream says which it is
    src = torch.from_numpy(hs).to(eng.dev)
    dst = torch.full((n * dstride,), CANARY, dtype=torch.uint8, device=eng.dev)
    j = np.zeros(n, SJ)
    idx = np.arange(n, dtype=np.uint64)
    j["src"], j["dst"] = np.uint64(src.data_ptr()) + idx * np.uint64(stride), np.uint64(dst.data_ptr()) + idx * np.uint64(dstride)
    j["src_len"], j["dst_cap"] = lens, dstride
    assert eng.deflate_stream_bound(48, 0, ZLIB) <= dstride
    rc, res = eng.deflate_stream_jobs(FHT, ZLIB, j)
    assert rc == 0
    r = eng.results_to_host(res, SR)
    out = dst.cpu().numpy().reshape(n, dstride)
    assert (r["cc"] == 0).all() and (r["blocks"] == 1).all()
    for i in range(n):
        data = hs[i, :lens[i]].tobytes()
        assert zlib.decompress(out[i, :r["out_len"][i]].tobytes()) == data, i       # (stream 65536 + k is not stream k: the first four bytes)
        assert r["adler"][i] == zlib.adler32(data), i
        assert (out[i, r["out_len"][i]:] == CANARY).all(), i


def test_refusals(eng):
    bufs = [make_block(k, n, seed=i) for i, (k, n) in enumerate([("alice", 70000), ("lz", 5000), ("zeros", 100), ("random", 3000),
                                                                  ("alice", 65536), ("lz", 200000), ("alice", 10), ("zeros", 0)])]
    run = Run(eng, DHTGEN, ZLIB, bufs, cap_delta=[0, -1, 0, 0, 0, 0, 0, 0], src_off=[0, 0, 0, 8, 0, 0, 0, 0], null_dst=(5,))
    assert run.rc == 0
    assert list(run.res["cc"]) == [0, 13, 0, 8, 0, 8, 0, 0]
    assert run.res["out_len"][1] == run.bound[1] and run.res["out_len"][3] == 0 and run.res["out_len"][5] == 0
    assert (run.res["blocks"][[1, 3, 5]] == 0).all()
    for i in (1, 3, 5):
        assert run.untouched(i, 0), i
    for i in (0, 2, 4, 6, 7):
        s = check_stream(run, i, ZLIB, bufs[i], 65536)
        assert s == framed(ZLIB, -1, host_stream(eng, DHTGEN, bufs[i], 0), bufs[i])
    # a function code that is no stream's
    j = np.zeros(1, SJ)
    assert eng.deflate_stream_jobs(DHT, ZLIB, j)[0] == -errno.EINVAL
    assert eng.deflate_stream_jobs(FHT, 3, j)[0] == -errno.EINVAL
    assert eng.deflate_stream_jobs(FHT, ZLIB, j, level=10)[0] == -errno.EINVAL


def test_unaligned_targets(eng):
    bufs = [make_block("alice", 70000, 1), make_block("lz", 65536, 2), make_block("random", 65536, 3), make_block("zeros", 131072 + 9, 4),
            mixed(3 * 65536 + 100, 5)]
    for fmt in (RAW, GZIP):
        base = Run(eng, DHTGEN, fmt, bufs)
        run = Run(eng, DHTGEN, fmt, bufs, dst_off=[1, 2, 3, 5, 7])
        assert base.rc == 0 and run.rc == 0 and run.res.tobytes() == base.res.tobytes()
        for i, b in enumerate(bufs):
            assert check_stream(run, i, fmt, b, 65536) == base.stream(i), i


def test_back_through_the_device_decoders(eng):
    import torch
    hist_max = 4096
    bufs = edge_buffers(hist_max)
    for fmt in (GZIP, ZLIB):
        run = Run(eng, DHTGEN, fmt, bufs, hist_max)
        assert run.rc == 0 and (run.res["cc"] == 0).all()
        n = len(bufs)
        jobs = np.zeros(n, pkg.JOB_DTYPE)
        jobs["src"] = np.uint64(run.dst.data_ptr()) + np.array(run.dat, np.uint64)
        jobs["src_len"] = run.res["out_len"]
        jobs["dst_cap"] = 0xffffffff
        res, frames = eng.decompress_size_framed(fmt, eng.to_device(jobs), n)
        r, f = eng.results_to_host(res), eng.frames_to_host(frames)
        assert (f["status"] == pkg.engine.FRAME_OK).all(), f["status"]
        assert list(r["tpbc"]) == [len(b) for b in bufs]
        at = np.concatenate([[0], np.cumsum((r["tpbc"].astype(np.int64) + 15) & ~15)])
        back = torch.zeros(int(at[-1]) + 16, dtype=torch.uint8, device=eng.dev)
        jobs["dst"] = np.uint64(back.data_ptr()) + at[:-1].astype(np.uint64)
        jobs["dst_cap"] = r["tpbc"]
        res, frames = eng.decompress_framed(fmt, eng.to_device(jobs), n)
        r, f = eng.results_to_host(res), eng.frames_to_host(frames)
        assert (f["status"] == pkg.engine.FRAME_OK).all(), f["status"]
        assert list(r["tpbc"]) == [len(b) for b in bufs]
        bk = back.cpu().numpy()
        for i, b in enumerate(bufs):
            assert bk[at[i]:at[i] + len(b)].tobytes() == b, i
