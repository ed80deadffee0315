"""GPU tests of nxz_batch_deflate_streams_dict (include/nxz_engine.h; the kernels in power-gzip_amd/csrc/nxz_streams_dict.hip, the rules
in nxz_streams_dict.h): a batch of device buffers of any length, each written as one raw or zlib stream whose first block sees a
shared preset dictionary.  The yardsticks are nxz_deflate_host_hist with prev = the dictionary -- the engine's own host-buffer path,
whose raw stream the deflate data must equal byte for byte --, zlib with inflateSetDictionary(the whole dictionary), the plain call
nxz_batch_deflate_streams where no block has a dictionary window, and the device decoders that take a dictionary."""
import ctypes as C
import errno
import importlib
import struct
import zlib

import numpy as np
import pytest

from datagen import make_block

pytestmark = pytest.mark.gpu
pkg = importlib.import_module("power-gzip_amd")
RAW, ZLIB, GZIP = pkg.engine.FMT_RAW, pkg.engine.FMT_ZLIB, pkg.engine.FMT_GZIP
SJ, SR = pkg.engine.STREAM_JOB_DTYPE, pkg.engine.STREAM_RESULT_DTYPE
FHT, DHTGEN = pkg.FC_COMPRESS_FHT, pkg.FC_COMPRESS_DHTGEN
WBITS = {RAW: -15, ZLIB: 15}
CANARY, TAIL = 0xc3, 64
FLG_FDICT = {-1: 0xbb, 1: 0x3f, 5: 0x7d, 6: 0xbb, 9: 0xf9}      # FLEVEL from the level, FDICT, FCHECK (tests/test_streams_dict_rules_host.py holds them against zlib)


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


def jsonish(n, seed):
    rows, i = [], seed * 1000
    while sum(map(len, rows)) < n:
        rows.append(b'{"id": %d, "name": "user%d", "active": %s, "tags": ["a%d", "b"], "score": %d.%d}\n'
                    % (i, i % 97, b"true" if i % 3 else b"false", i % 7, i * 31 % 1000, i % 10))
        i += 1
    return b"".join(rows)[:n]


_dicts = {}


def dictionary(n):
    """n bytes the buffers below share vocabulary with: text, then JSON-like rows"""
    if n not in _dicts:
        _dicts[n] = make_block("alice", n // 2, 40) + jsonish(n - n // 2, 7)
        assert len(_dicts[n]) == n
    return _dicts[n]


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
    bufs = [b"", make_block("alice", 1, 1), jsonish(15, 2), jsonish(16, 3), make_block("alice", B - 1, 4), make_block("random", B, 5),
            jsonish(B + 1, 6), mixed(2 * B + 17, 8), mixed(3 * B + 5, 9)]
    assert [len(b) for b in bufs] == [0, 1, 15, 16, B - 1, B, B + 1, 2 * B + 17, 3 * B + 5]
    return bufs


_ref = {}


def host_stream(eng, fc, data, hist_max, prev):
    """the raw deflate stream nxz_deflate_host_hist writes for `data` (final) with `prev` as the earlier input -- the parent's code"""
    key = (fc, hist_max, hash(data), len(data), hash(prev), len(prev or b""))
    if key not in _ref:
        if not data:
            _ref[key] = bytes.fromhex("010000ffff")          # (the host call takes no empty buffer)
        else:
            cap = eng.L.nxz_deflate_host_bound_hist(len(data), hist_max)
            dst = C.create_string_buffer(cap)
            n, crc, adler = C.c_size_t(), C.c_uint32(), C.c_uint32()
            rc = eng.L.nxz_deflate_host_hist(eng.ctx, fc, data, len(data), 1, hist_max, prev if prev else None, len(prev) if prev else 0,
                                             dst, cap, C.byref(n), C.byref(crc), C.byref(adler))
            assert rc == 0 and crc.value == zlib.crc32(data) and adler.value == zlib.adler32(data)
            _ref[key] = dst.raw[:n.value]
    return _ref[key]


def header(fmt, level, dict_bytes):
    return bytes([0x78, FLG_FDICT[level]]) + struct.pack(">I", zlib.adler32(dict_bytes)) if fmt == ZLIB else b""


def framed(fmt, level, dict_bytes, body, data):
    return header(fmt, level, dict_bytes) + body + (struct.pack(">I", zlib.adler32(data)) if fmt == ZLIB else b"")


def body_of(fmt, stream):
    return stream[6:-4] if fmt == ZLIB else stream


class Run:
    """one call: sources at 16-byte aligned offsets of one device buffer, targets in slots of one device buffer filled with canary
    bytes.  d: a Dict, None for the plain call nxz_batch_deflate_streams, or "null" for the dictionary call with dict = NULL"""

    def __init__(self, eng, fc, fmt, d, bufs, hist_max=0, level=-1, dst_off=None, cap_delta=None, src_off=None, null_dst=()):
        import torch
        n = len(bufs)
        dst_off = dst_off or [0] * n
        cap_delta = cap_delta or [0] * n
        src_off = src_off or [0] * n
        bound = eng.deflate_stream_bound if d is None else eng.deflate_stream_bound_dict
        self.bound = [bound(len(b), hist_max, fmt) for b in bufs]
        self.cap = [b + x for b, x in zip(self.bound, cap_delta)]
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
        if d is None:
            self.rc, res = eng.deflate_stream_jobs(fc, fmt, j, hist_max=hist_max, level=level)
        else:
            self.rc, res = eng.deflate_stream_jobs_dict(fc, fmt, None if isinstance(d, str) else d, j, hist_max=hist_max, level=level)
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


def check_stream(run, i, fmt, dict_bytes, data, B):
    r = run.res[i]
    assert r["cc"] == 0, (i, r)
    s = run.stream(i)
    z = zlib.decompressobj(WBITS[fmt], zdict=dict_bytes) if dict_bytes else zlib.decompressobj(WBITS[fmt])
    if fmt == ZLIB and not dict_bytes:
        # zlib takes no empty dictionary and so cannot answer a stream that asks for one: its deflate data alone
        assert s[:6] == bytes([0x78, s[1], 0, 0, 0, 1]) and s[1] & 0x20 and (0x7800 + s[1]) % 31 == 0, i
        assert s[-4:] == struct.pack(">I", zlib.adler32(data)), i
        z, s_in = zlib.decompressobj(-15), s[6:-4]
    else:
        s_in = s
    assert z.decompress(s_in) == data and z.eof and z.unused_data == b"", i
    assert r["crc"] == zlib.crc32(data) and r["adler"] == zlib.adler32(data), (i, r)
    assert r["blocks"] == (len(data) + B - 1) // B and r["out_len"] <= run.bound[i], (i, r)
    assert run.untouched(i, int(r["out_len"])), i
    return s


@pytest.mark.parametrize("fmt", [RAW, ZLIB])
@pytest.mark.parametrize("dl", [0, 16, 17, 4101, 32768, 40000])
@pytest.mark.parametrize("hist_max", [4096, 32768])
@pytest.mark.parametrize("fc", [FHT, DHTGEN])
def test_edges_of_the_cut(eng, fc, hist_max, dl, fmt):
    B, dict_bytes, level = block_bytes(hist_max), dictionary(dl), 5
    bufs = edge_buffers(hist_max)
    assert pkg.engine.stream_dict_window(dl, hist_max) == min(hist_max, dl) & ~15
    for b in bufs:
        assert eng.deflate_stream_bound_dict(len(b), hist_max, fmt) == eng.deflate_stream_bound(len(b), hist_max, fmt) + (4 if fmt == ZLIB else 0)
    d = eng.dict_create(dict_bytes)
    try:
        run = Run(eng, fc, fmt, d, bufs, hist_max, level)
        assert run.rc == 0
        for i, b in enumerate(bufs):
            s = check_stream(run, i, fmt, dict_bytes, b, B)
            assert s == framed(fmt, level, dict_bytes, host_stream(eng, fc, b, hist_max, dict_bytes), b), "stream %d is not nxz_deflate_host_hist's" % i
        assert run.res["stored"][0] == 0 and run.res["stored"][5] >= 1 and run.res["blocks"][8] == 4
    finally:
        d.close()


def test_the_dictionary_is_really_the_window(eng):
    hist_max = 32768
    dict_bytes = make_block("random", 32768, 21)
    data = dict_bytes[-1000:] + jsonish(300, 3)
    for fc in (FHT, DHTGEN):
        ref, alone = host_stream(eng, fc, data, hist_max, dict_bytes), host_stream(eng, fc, data, hist_max, None)
        assert len(ref) < len(alone) - 900                     # 1000 random bytes as a few matches into the dictionary
        with pytest.raises(zlib.error):
            zlib.decompressobj(-15).decompress(ref)            # distances that reach in front of the stream
        assert zlib.decompressobj(-15, zdict=dict_bytes).decompress(ref) == data
        d = eng.dict_create(dict_bytes)
        try:
            run = Run(eng, fc, RAW, d, [data], hist_max)
            assert run.rc == 0 and check_stream(run, 0, RAW, dict_bytes, data, 32768) == ref
        finally:
            d.close()


def test_hist_max_0_names_the_dictionary_and_does_not_use_it(eng):
    dict_bytes = dictionary(32768)
    bufs = [b"", dict_bytes[-1000:], jsonish(3000, 1), mixed(65536 + 70000, 2)]
    d = eng.dict_create(dict_bytes)
    try:
        for fc in (FHT, DHTGEN):
            plain = Run(eng, fc, RAW, None, bufs)
            for fmt in (RAW, ZLIB):
                run = Run(eng, fc, fmt, d, bufs, 0, 9)
                assert plain.rc == 0 and run.rc == 0
                for i, b in enumerate(bufs):
                    s = check_stream(run, i, fmt, dict_bytes, b, 65536)
                    assert body_of(fmt, s) == plain.stream(i), i
                    assert s == framed(fmt, 9, dict_bytes, plain.stream(i), b), i
    finally:
        d.close()


@pytest.mark.parametrize("hist_max", [0, 4096, 32768])
def test_empty_dictionary_is_the_plain_call(eng, hist_max):
    bufs = edge_buffers(hist_max)
    d = eng.dict_create(b"")
    try:
        assert d.id == 1
        plain = Run(eng, DHTGEN, RAW, None, bufs, hist_max)
        for fmt in (RAW, ZLIB):
            run = Run(eng, DHTGEN, fmt, d, bufs, hist_max, 1)
            assert plain.rc == 0 and run.rc == 0
            for i, b in enumerate(bufs):
                s = check_stream(run, i, fmt, b"", b, block_bytes(hist_max))
                assert body_of(fmt, s) == plain.stream(i), i
                if fmt == ZLIB:
                    assert s[:6] == bytes.fromhex("783f00000001"), i
    finally:
        d.close()


def test_chunks_do_not_show(eng, monkeypatch):
    hist_max = 32768
    dict_bytes = dictionary(40000)
    # first blocks at the batch's blocks 0, 1, 2, 6, 8 and 12 to 19 of 22: chunks of 3 hold none, one, two or three of them, and streams straddle chunks
    bufs = ([jsonish(500, 1), make_block("alice", 32768, 2), mixed(4 * 32768 - 1, 3), b"", jsonish(32769, 4), mixed(3 * 32768 + 5, 5)]
            + [jsonish(700 + 17 * k, 20 + k) for k in range(7)] + [mixed(2 * 32768 + 17, 6)])
    d = eng.dict_create(dict_bytes)
    try:
        monkeypatch.delenv("NXZ_STREAMS_CHUNK", raising=False)
        base = Run(eng, DHTGEN, ZLIB, d, bufs, hist_max)
        assert base.rc == 0 and (base.res["cc"] == 0).all() and list(base.res["blocks"][:6]) == [1, 1, 4, 0, 2, 4]
        for i, b in enumerate(bufs):
            s = check_stream(base, i, ZLIB, dict_bytes, b, 32768)
            assert body_of(ZLIB, s) == host_stream(eng, DHTGEN, b, hist_max, dict_bytes), i
        for chunk in (1, 3, 5):
            monkeypatch.setenv("NXZ_STREAMS_CHUNK", str(chunk))
            run = Run(eng, DHTGEN, ZLIB, d, bufs, hist_max)
            assert run.rc == 0
            assert run.res.tobytes() == base.res.tobytes(), chunk
            assert np.array_equal(run.out, base.out), chunk
    finally:
        d.close()


def test_many_small_streams(eng):
    import torch
    n, stride, hist_max = 1024, 2048, 32768
    dict_bytes = jsonish(32768, 7)
    rnd = np.random.default_rng(11)
    lens = rnd.integers(100, 2001, n)
    records = [jsonish(int(lens[i]), 100 + i) for i in range(n)]
    hs = np.zeros((n, stride), np.uint8)
    for i, r in enumerate(records):
        hs[i, :len(r)] = np.frombuffer(r, np.uint8)
    dstride = (eng.deflate_stream_bound_dict(2000, hist_max, ZLIB) + 15) & ~15
    src = torch.from_numpy(hs).to(eng.dev)
    dst = torch.full((n * dstride,), CANARY, dtype=torch.uint8, device=eng.dev)
    j = np.zeros(n, SJ)
    idx = np.arange(n, dtype=np.uint64)
    j["src"], j["dst"] = np.uint64(src.data_ptr()) + idx * np.uint64(stride), np.uint64(dst.data_ptr()) + idx * np.uint64(dstride)
    j["src_len"], j["dst_cap"] = lens, dstride
    d = eng.dict_create(dict_bytes)
    try:
        rc, res = eng.deflate_stream_jobs_dict(DHTGEN, ZLIB, d, j, hist_max=hist_max)
        assert rc == 0
        r = eng.results_to_host(res, SR)
        out = dst.cpu().numpy().reshape(n, dstride)
        assert (r["cc"] == 0).all() and (r["blocks"] == 1).all()
        for i, data in enumerate(records):
            s = out[i, :r["out_len"][i]].tobytes()
            z = zlib.decompressobj(zdict=dict_bytes)
            assert z.decompress(s) == data and z.eof and z.unused_data == b"", i
            assert r["adler"][i] == zlib.adler32(data) and (out[i, r["out_len"][i]:] == CANARY).all(), i
            if i % 16 == 0:
                assert s == framed(ZLIB, -1, dict_bytes, host_stream(eng, DHTGEN, data, hist_max, dict_bytes), data), i
    finally:
        d.close()


def test_refusals_among_good_streams(eng):
    hist_max = 32768
    dict_bytes = dictionary(32768)
    bufs = [make_block(k, n, seed=i) for i, (k, n) in enumerate([("alice", 70000), ("lz", 5000), ("zeros", 100), ("random", 3000),
                                                                  ("alice", 32768), ("lz", 100000), ("alice", 10), ("zeros", 0)])]
    d = eng.dict_create(dict_bytes)
    try:
        run = Run(eng, DHTGEN, ZLIB, d, bufs, hist_max, cap_delta=[0, -1, 0, 0, 0, 0, 0, 0], src_off=[0, 0, 0, 8, 0, 0, 0, 0], null_dst=(5,))
        assert run.rc == 0
        assert list(run.res["cc"]) == [0, 13, 0, 8, 0, 8, 0, 0]
        assert run.res["out_len"][1] == run.bound[1] == eng.deflate_stream_bound(5000, hist_max, ZLIB) + 4
        assert run.res["out_len"][3] == 0 and run.res["out_len"][5] == 0 and (run.res["blocks"][[1, 3, 5]] == 0).all()
        for i in (1, 3, 5):
            assert run.untouched(i, 0), i
        for i in (0, 2, 4, 6, 7):
            s = check_stream(run, i, ZLIB, dict_bytes, bufs[i], 32768)
            assert s == framed(ZLIB, -1, dict_bytes, host_stream(eng, DHTGEN, bufs[i], hist_max, dict_bytes), bufs[i]), i
        # what the call does not take at all
        j = np.zeros(1, SJ)
        assert eng.deflate_stream_jobs_dict(FHT, GZIP, d, j)[0] == -errno.EINVAL
        assert eng.deflate_stream_jobs_dict(FHT, ZLIB, None, j)[0] == -errno.EINVAL
        assert eng.deflate_stream_jobs_dict(pkg.FC_COMPRESS_DHT, ZLIB, d, j)[0] == -errno.EINVAL
        assert eng.deflate_stream_jobs_dict(FHT, ZLIB, d, j, level=10)[0] == -errno.EINVAL
        assert eng.deflate_stream_bound_dict(1000, hist_max, GZIP) == 0
    finally:
        d.close()


def test_unaligned_targets(eng):
    hist_max = 4096
    dict_bytes = dictionary(4101)
    B = block_bytes(hist_max)
    bufs = [make_block("alice", 70000, 1), make_block("lz", B, 2), make_block("random", B, 3), make_block("zeros", 2 * B + 9, 4), jsonish(900, 5)]
    d = eng.dict_create(dict_bytes)
    try:
        for fmt in (RAW, ZLIB):
            base = Run(eng, DHTGEN, fmt, d, bufs, hist_max)
            run = Run(eng, DHTGEN, fmt, d, bufs, hist_max, dst_off=[1, 2, 3, 5, 7])
            assert base.rc == 0 and run.rc == 0 and run.res.tobytes() == base.res.tobytes()
            for i, b in enumerate(bufs):
                assert check_stream(run, i, fmt, dict_bytes, b, B) == base.stream(i), i
    finally:
        d.close()


def test_back_through_the_device_decoders(eng):
    import torch
    hist_max = 4096
    dict_bytes = dictionary(32768)
    bufs = edge_buffers(hist_max)[:-1]                          # up to 2 * B + 17 bytes
    n = len(bufs)
    d = eng.dict_create(dict_bytes)
    try:
        for fmt in (ZLIB, RAW):
            run = Run(eng, DHTGEN, fmt, d, bufs, hist_max)
            assert run.rc == 0 and (run.res["cc"] == 0).all()
            at = np.concatenate([[0], np.cumsum([(len(b) + 31) & ~15 for b in bufs])])
            back = torch.zeros(int(at[-1]) + 16, dtype=torch.uint8, device=eng.dev)
            jobs = np.zeros(n, pkg.JOB_DTYPE)
            jobs["src"] = np.uint64(run.dst.data_ptr()) + np.array(run.dat, np.uint64)
            jobs["src_len"] = run.res["out_len"]
            jobs["dst"] = np.uint64(back.data_ptr()) + at[:-1].astype(np.uint64)
            jobs["dst_cap"] = [len(b) for b in bufs]
            jobs["in_adler"] = 1
            if fmt == ZLIB:
                res, frames = eng.decompress_framed_dict(ZLIB, d, eng.to_device(jobs), n)
                f = eng.frames_to_host(frames)
                assert (f["status"] == pkg.FRAME_OK).all() and (f["hdr_len"] == 6).all() and (f["dictid"] == d.id).all(), f
            else:
                res = eng.decompress_dict(d, eng.to_device(jobs), n)
            r = eng.results_to_host(res)
            assert (r["cc"][:n] == 0).all() and list(r["tpbc"][:n]) == [len(b) for b in bufs], r
            bk = back.cpu().numpy()
            for i, b in enumerate(bufs):
                assert bk[at[i]:at[i] + len(b)].tobytes() == b, i
    finally:
        d.close()
