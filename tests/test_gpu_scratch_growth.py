"""GPU tests of the per-stream scratch of the batched interface (power-gzip_amd/csrc/nxz_ctx.h: DevBuf, nxz_ctx::Scratch): every
grow-only buffer is sized by a small batch, has to grow for a larger one and is kept for the small one again, all on ONE engine
stream of nxz_stream_create.  A buffer that is kept when it should grow is too small for the larger batch, one that is freed
without the stream's wait goes away under the kernels of the batch before, and one that is regrown without its "new" flag holds
no tables: each shows as a wrong output here.  Every output is compared with the CPU oracle or with zlib.  Streams and sources
are tiny (a few hundred to 4096 bytes), so a case takes a second or two."""
import ctypes as C
import gzip
import importlib
import os
import zlib

import numpy as np
import pytest

import bgzf_model as M
import framing as F
import oracle_lib as O
from datagen import make_block

pytestmark = pytest.mark.gpu
pkg = importlib.import_module("power-gzip_amd")
KNOBS = ("NXZ_INFLATE_LANES_MIN", "NXZ_INFLATE_CUT", "NXZ_INFLATE_WG", "NXZ_INFLATE_WG_MAX", "NXZ_WG_PMIN", "NXZ_INFLATE_ORDER",
         "NXZ_FUSED_GEN", "NXZ_COMPRESS_CHUNK", "NXZ_DICT_WG_MIN", "NXZ_BGZF_CHUNK")
KINDS = ["alice", "lz", "text33", "zeros", "random"]


class OnStream:
    """an engine whose calls go to one stream of nxz_stream_create instead of torch's current stream.  torch knows nothing of that
    stream: what torch has queued is waited for before every engine call, and the whole device before anything is read back
    (results_to_host and frames_to_host do that, the BGZF calls wait for their stream themselves)."""

    def __init__(self, eng):
        import torch
        self.eng, self.torch = eng, torch
        eng.L.nxz_stream_create.restype = C.c_void_p
        eng.L.nxz_stream_create.argtypes = [C.c_void_p]
        eng.L.nxz_stream_destroy.argtypes = [C.c_void_p, C.c_void_p]
        self.handle = eng.L.nxz_stream_create(eng.ctx)
        assert self.handle
        eng.stream_handle = self._stream_handle

    def _stream_handle(self):
        self.torch.cuda.synchronize(self.eng.dev)
        return C.c_void_p(self.handle)

    def destroy(self):
        if self.handle:
            self.eng.L.nxz_stream_destroy(self.eng.ctx, C.c_void_p(self.handle))
            self.handle = None
        self.eng.__dict__.pop("stream_handle", None)


@pytest.fixture
def eng():
    saved = {k: os.environ.pop(k, None) for k in KNOBS}
    e = pkg.Engine(0)
    s = OnStream(e)
    yield e
    s.destroy()
    e.close()
    for k in KNOBS:
        os.environ.pop(k, None)
    for k, v in saved.items():
        if v is not None:
            os.environ[k] = v


def sources(n, seed):
    """n sources of 200 .. 4096 bytes of every kind"""
    rng = np.random.RandomState(seed)
    return [make_block(KINDS[i % 5], int(rng.randint(200, 4097)), seed=seed + i) for i in range(n)]


def place(eng, bufs):
    """bufs in one device tensor, each at a 16-byte aligned place; returns (tensor, device addresses)"""
    import torch
    at, total = [], 0
    for b in bufs:
        at.append(total)
        total += (len(b) + 16 + 15) & ~15
    host = np.full(max(total, 16), 0xa5, np.uint8)
    for b, a in zip(bufs, at):
        host[a:a + len(b)] = np.frombuffer(b, np.uint8)
    t = torch.from_numpy(host).to(eng.dev)
    return t, np.uint64(t.data_ptr()) + np.array(at, np.uint64)


def targets(eng, caps):
    import torch
    at, total = [], 0
    for c in caps:
        at.append(total)
        total += (c + 16 + 15) & ~15
    return torch.full((max(total, 16),), 0xcd, dtype=torch.uint8, device=eng.dev), np.array(at, np.int64)


def make_jobs(eng, src_addr, src_lens, dst_t, dst_at, caps, dht_index=None):
    j = np.zeros(len(src_lens), pkg.JOB_DTYPE)
    j["src"] = src_addr
    j["dst"] = np.uint64(dst_t.data_ptr()) + dst_at.astype(np.uint64)
    j["src_len"] = src_lens
    j["dst_cap"] = caps
    j["in_adler"] = 1
    if dht_index is not None:
        j["dht_index"] = dht_index
    return eng.to_device(j)


def own_table(data, hist=0):
    """the oracle's table for the block's own counts"""
    tok, nt = O.lz77(data, hist)
    ll, d = O.counts(tok, nt)
    return O.dhtgen(ll, d)


def compress_check(eng, fc, srcs, tables=None, d=None, dict_bytes=b""):
    """srcs through nxz_batch_compress[_dict]; every block equals the oracle's and inflates to its source with zlib"""
    n = len(srcs)
    W = d.deflate_window if d else 0
    window = dict_bytes[len(dict_bytes) - W:] if W else b""
    caps = [int(eng.L.nxz_compress_bound(len(s))) + 512 for s in srcs]
    st, saddr = place(eng, srcs)
    dt, dat = targets(eng, caps)
    dht = None
    if tables:
        arr = np.zeros(len(tables), pkg.DHT_DTYPE)
        for i, (bits, k) in enumerate(tables):
            arr["dhtlen"][i] = k
            arr["dht"][i, :len(bits)] = np.frombuffer(bits, np.uint8)
        dht = eng.to_device(arr)
    jobs = make_jobs(eng, saddr, [len(s) for s in srcs], dt, dat, caps, dht_index=np.arange(n) % len(tables) if tables else None)
    if d:
        res, _ = eng.compress_dict(fc, d, jobs, n, dht=dht, ntables=len(tables) if tables else 0)
    else:
        res, _ = eng.compress(fc, jobs, n, dht=dht, ntables=len(tables) if tables else 0)
    r = eng.results_to_host(res)
    out = dt.cpu().numpy()
    for i, s in enumerate(srcs):
        a, k = int(dat[i]), int(r["tpbc"][i])
        got = out[a:a + k].tobytes()
        table = tables[i % len(tables)] if tables else own_table(window + s, W)
        exp, bits = O.deflate_dynamic(window + s, table[0], table[1], hist=W)
        assert r["cc"][i] in (0, 64) and got == exp and r["tebc"][i] == bits % 8, (n, i, r[i])    # (64: more bytes out than in)
        assert r["crc"][i] == zlib.crc32(s) and r["adler"][i] == zlib.adler32(s), (n, i)
        z = zlib.decompressobj(-15, zdict=dict_bytes) if dict_bytes else zlib.decompressobj(-15)
        assert z.decompress(got) == s, (n, i)


def raw_streams(n, seed, zdict=b""):
    plains = sources(n, seed)
    out = []
    for i, p in enumerate(plains):
        level = [1, 6, 9][i % 3]
        c = zlib.compressobj(level, zlib.DEFLATED, -15, 8, zlib.Z_DEFAULT_STRATEGY, zdict) if zdict else zlib.compressobj(level, zlib.DEFLATED, -15)
        out.append(c.compress(p) + c.flush())
    return plains, out


def inflate_check(eng, n, seed, d=None, dict_bytes=b""):
    """n zlib-made raw streams through nxz_batch_decompress[_dict]; every output equals its plain text"""
    plains, streams = raw_streams(n, seed, dict_bytes)
    caps = [len(p) for p in plains]
    st, saddr = place(eng, streams)
    dt, dat = targets(eng, caps)
    jobs = make_jobs(eng, saddr, [len(s) for s in streams], dt, dat, caps)
    res = eng.decompress_dict(d, jobs, n) if d else eng.decompress(jobs, n)
    r = eng.results_to_host(res)
    out = dt.cpu().numpy()
    for i, p in enumerate(plains):
        a = int(dat[i])
        assert r["cc"][i] == 0 and r["tpbc"][i] == len(p), (n, i, r[i])
        assert out[a:a + len(p)].tobytes() == p, (n, i)
        assert r["crc"][i] == zlib.crc32(p) and r["adler"][i] == zlib.adler32(p), (n, i)


def caller_tables(eng):
    """nxz_batch_compress with the caller's tables (the prepared tables grow): 1 table, then 3, then 1"""
    for k in (1, 3, 1):
        srcs = sources(k, 10 + k)
        compress_check(eng, pkg.FC_COMPRESS_DHT, srcs, tables=[own_table(s) for s in srcs])


def test_compress_caller_tables(eng):
    caller_tables(eng)


def test_compress_dhtgen_and_trim(eng):
    """the chunk of tokens, tables and counts (the chunk is the batch at these sizes): 2 jobs, then 40; nxz_trim() gives it back,
    and 2 jobs get a new one"""
    compress_check(eng, pkg.FC_COMPRESS_DHTGEN, sources(2, 20))
    compress_check(eng, pkg.FC_COMPRESS_DHTGEN, sources(40, 21))
    eng.torch.cuda.synchronize(eng.dev)
    eng.L.nxz_trim.restype = C.c_size_t
    assert eng.L.nxz_trim() > 0
    compress_check(eng, pkg.FC_COMPRESS_DHTGEN, sources(2, 20))


def test_compress_dict(eng):
    """nxz_batch_compress_dict (the rewritten jobs grow, and the chunk): 2 jobs, then 40, then 2"""
    dict_bytes = make_block("alice", 5000, seed=3)
    d = eng.dict_create(dict_bytes)
    try:
        for n in (2, 40, 2):
            compress_check(eng, pkg.FC_COMPRESS_DHTGEN, sources(n, 30 + n), d=d, dict_bytes=dict_bytes)
    finally:
        eng.torch.cuda.synchronize(eng.dev)
        d.close()


def test_inflate_a_workgroup_each(eng):
    """the default route (the workgroup kernel's workspace; from 128 streams on the order workspace): 2, then 130, then 2 streams"""
    for n in (2, 130, 2):
        inflate_check(eng, n, 40 + n)
        assert eng.wg_reasons() is not None, n                      # (the workgroup kernel's workspace is there: the batch went that way)


def test_inflate_dict(eng):
    """nxz_batch_decompress_dict, the same workspaces: 2, then 130, then 2 streams (all through the workgroup kernel)"""
    os.environ["NXZ_DICT_WG_MIN"] = "0"
    dict_bytes = make_block("alice", 5000, seed=4)
    d = eng.dict_create(dict_bytes)
    try:
        for n in (2, 130, 2):
            inflate_check(eng, n, 50 + n, d=d, dict_bytes=dict_bytes)
    finally:
        eng.torch.cuda.synchronize(eng.dev)
        d.close()


def test_inflate_a_stream_per_lane(eng):
    """NXZ_INFLATE_WG=0, NXZ_INFLATE_LANES_MIN=1: 8, then 40, then 8 streams.  nxz_inflate_lanes_workspace (nxz_inflate_lanes.hip)
    holds 65 table slots per resident wavefront and one more, and a wavefront takes 32 streams at these sizes: 8 streams are one
    wavefront (66 slots), 40 are two (131 slots), so the second batch gets a new workspace -- whose tables have to be made again
    (init = 1): a regrown workspace that is not initialised decodes fixed-code blocks with whatever the allocation held."""
    os.environ["NXZ_INFLATE_WG"] = "0"
    os.environ["NXZ_INFLATE_LANES_MIN"] = "1"
    for n in (8, 40, 8):
        inflate_check(eng, n, 60 + n)


def test_inflate_cut_into_pieces(eng):
    """NXZ_INFLATE_WG=0, NXZ_INFLATE_CUT=1 (the cut workspace: control arrays per stream, then the arena): 1 stream, then 8, then 1"""
    os.environ["NXZ_INFLATE_WG"] = "0"
    os.environ["NXZ_INFLATE_CUT"] = "1"
    for n in (1, 8, 1):
        inflate_check(eng, n, 70 + n)


def test_inflate_a_stream_per_wavefront_with_order(eng):
    """NXZ_INFLATE_WG=0, NXZ_INFLATE_ORDER=1 (the order workspace of the stream-per-wavefront route): 2 streams, then 40, then 2"""
    os.environ["NXZ_INFLATE_WG"] = "0"
    os.environ["NXZ_INFLATE_ORDER"] = "1"
    for n in (2, 40, 2):
        inflate_check(eng, n, 80 + n)


def test_framed_gzip(eng):
    """nxz_batch_decompress_framed (the derived jobs grow): 2 gzip members, then 40, then 2"""
    for n in (2, 40, 2):
        plains = sources(n, 90 + n)
        members = [F.gzip_member(p, [1, 6, 9][i % 3]) for i, p in enumerate(plains)]
        caps = [len(p) for p in plains]
        mt, maddr = place(eng, members)
        dt, dat = targets(eng, caps)
        res, fr = eng.decompress_framed(pkg.FMT_GZIP, make_jobs(eng, maddr, [len(m) for m in members], dt, dat, caps), n)
        r, f = eng.results_to_host(res), eng.frames_to_host(fr)
        out = dt.cpu().numpy()
        for i, p in enumerate(plains):
            assert f["status"][i] == pkg.FRAME_OK and f["end"][i] == len(members[i]) and f["check"][i] == zlib.crc32(p), (n, i, f[i])
            assert r["cc"][i] == 0 and r["tpbc"][i] == len(p) and out[int(dat[i]):int(dat[i]) + len(p)].tobytes() == p, (n, i, r[i])


def test_bgzf_unpack_index_and_ranges(eng):
    """nxz_batch_unpack_gzip, nxz_bgzf_index (the discovery's workspace and the candidates it has room for) and
    nxz_bgzf_read_ranges (the map's arrays; the slots, used over several chunks with NXZ_BGZF_CHUNK=8): an image of 2 members
    with 1 range, then one of 40 members with 50 ranges, then the first again"""
    import torch
    os.environ["NXZ_BGZF_CHUNK"] = "8"
    rng = np.random.RandomState(7)
    for members, nranges in ((2, 1), (40, 50), (2, 1)):
        plains = sources(members, 100 + members)
        data = b"".join(plains)
        image = b"".join(M.member(p, [1, 6, 9][i % 3]) for i, p in enumerate(plains)) + M.EOF_MARKER
        assert gzip.decompress(image) == data
        host = np.zeros(len(image) + 16, np.uint8)
        host[:len(image)] = np.frombuffer(image, np.uint8)
        t = torch.from_numpy(host).to(eng.dev)
        dst = torch.full((len(data) + 16,), 0xcd, dtype=torch.uint8, device=eng.dev)
        rc, d = eng.unpack_gzip(t, len(image), dst, members + 8)
        assert rc == 0 and d["members"] == members + 1 and d["consumed"] == len(image) and d["out_len"] == len(data), (members, rc, d)
        assert dst.cpu().numpy()[:len(data)].tobytes() == data, members
        coff, uoff = eng.bgzf_index(t, len(image), members + 8)
        assert (coff.cpu().tolist(), uoff.cpu().tolist()) == M.index(image), members
        ranges = [(0, len(data))] if nranges == 1 else []
        while len(ranges) < nranges:
            b = int(rng.randint(0, len(data)))
            ranges.append((b, min(len(data), b + int(rng.randint(0, 9000)))))
        rt = torch.tensor(np.array(ranges, np.uint64).reshape(-1, 2).view(np.int64), device=eng.dev)
        rc, offs, st, out_len, decoded, got = eng.bgzf_read_ranges(t, len(image), coff, uoff, rt)
        torch.cuda.synchronize(eng.dev)
        offs, st, got = offs.cpu().numpy(), st.cpu().numpy(), got.cpu().numpy()
        assert rc == 0 and out_len == offs[-1] == sum(e - b for b, e in ranges) and 0 < decoded <= members, (members, rc, out_len, decoded)
        for i, (b, e) in enumerate(ranges):
            assert st[i] == M.OK and got[offs[i]:offs[i + 1]].tobytes() == data[b:e], (members, i, b, e)


def test_bgzf_and_checkpoint_ranges_take_turns(eng):
    """nxz_bgzf_read_ranges and nxz_checkpoint_read_ranges share BUF_RNG (the map's arrays) and BUF_RNG_SLOTS (a chunk's slots, jobs,
    frames and results): on one stream a BGZF image of 3 members, a zlib stream of 200 KiB through its index of 16 KiB spans, an
    image of 40 members, the zlib stream and the small image again -- the map's arrays grow with the members, the slots with the
    segments (16 KiB and more of output, and an input slot, where a member has 4 KiB at most), and each call gets what the other
    left.  NXZ_BGZF_CHUNK=3: every call with more than three members runs several chunks.  Eight ranges a call: an empty one, one
    inside a member, one over more than three, the ends; every byte against the plain slices."""
    import bisect
    import torch
    import checkpoint_model as CM
    os.environ["NXZ_BGZF_CHUNK"] = "3"
    dev = eng.dev

    def on_device(b):
        host = np.zeros(len(b) + 16, np.uint8)
        host[:len(b)] = np.frombuffer(b, np.uint8)
        return torch.from_numpy(host).to(dev)

    def eight(u, n):
        """u: the uncompressed offsets of the members (or segments), n: the plain length"""
        L, mid = len(u) - 1, (len(u) - 1) // 2
        r = [(7, 7), (u[mid] + 5, u[mid] + 105), (u[1] - 1, u[min(5, L)] + 1 if L >= 5 else n), (0, n), (n - 1, n), (0, 1),
             (u[mid + 1] - 3, min(n, u[mid + 1] + 3)), (u[mid] + 50, u[mid] + 80)]
        assert all(0 <= b <= e <= n for b, e in r) and (L < 5 or bisect.bisect_right(u, r[2][1] - 1) - bisect.bisect_right(u, r[2][0]) >= 4)
        return r

    def touched(u, ranges):
        out = set()
        for b, e in ranges:
            if b < e:
                out |= set(range(bisect.bisect_right(u[:-1], b) - 1, bisect.bisect_right(u[:-1], e - 1)))
        return len(out)

    def check(what, plain, u, ranges, rc, offs, st, out_len, decoded, got):
        torch.cuda.synchronize(dev)
        offs, st, got = offs.cpu().numpy(), st.cpu().numpy(), got.cpu().numpy()
        assert rc == 0 and out_len == offs[-1] == sum(e - b for b, e in ranges), (what, rc, out_len)
        assert decoded == touched(u, ranges) and (len(u) - 1 <= 3 or decoded > 3), (what, decoded)
        for i, (b, e) in enumerate(ranges):
            assert st[i] == pkg.RANGE_OK and got[offs[i]:offs[i + 1]].tobytes() == plain[b:e], (what, i, b, e)

    images = {}
    for members in (3, 40):
        plains = sources(members, 300 + members)
        assert max(len(p) for p in plains) <= 4096
        image = b"".join(M.member(p, [1, 6, 9][i % 3]) for i, p in enumerate(plains)) + M.EOF_MARKER
        t = on_device(image)
        coff, uoff = eng.bgzf_index(t, len(image), members + 8)
        assert (coff.cpu().tolist(), uoff.cpu().tolist()) == M.index(image), members
        images[members] = (b"".join(plains), image, t, coff, uoff)
    plain = b"".join(make_block(KINDS[k % 3], 65536, seed=40 + k) for k in range(3)) + make_block("alice", 8193, seed=44)
    stream = CM.deflate(plain, CM.FMT_ZLIB, 6, 1)
    m = CM.index(stream, CM.FMT_ZLIB, 16384)
    assert m["plain"] == plain and m["count"] >= 6
    src, out = on_device(stream), on_device(plain)
    j = np.zeros(1, pkg.JOB_DTYPE)
    j[0]["src"], j[0]["src_len"], j[0]["dst"], j[0]["dst_cap"], j[0]["in_adler"] = src.data_ptr(), len(stream), out.data_ptr(), len(plain), 1
    rc, cbit, cuoff, windows, streams = eng.checkpoint_index(pkg.FMT_ZLIB, eng.to_device(j), 1, 16384, m["count"], windows=True)
    rec = eng.results_to_host(streams, pkg.CHECKPOINT_STREAM_DTYPE)[0]
    assert rc == 0 and rec["status"] == pkg.CPS_OK and rec["count"] == m["count"]
    assert cuoff[0].cpu().tolist() == m["uoff"] and cbit[0].cpu().tolist() == m["cbit"]
    cbit, cuoff, windows = cbit[0].contiguous(), cuoff[0].contiguous(), windows[0].contiguous()

    for turn in (3, "zlib", 40, "zlib", 3):
        if turn == "zlib":
            ranges = eight(m["uoff"], len(plain))
            r = torch.tensor(np.array(ranges, np.int64), device=dev)
            check(turn, plain, m["uoff"], ranges, *eng.checkpoint_read_ranges(src, len(stream), cbit, cuoff, windows, r))
        else:
            data, image, t, coff, uoff = images[turn]
            u = M.index(image)[1]
            ranges = eight(u[:-1], len(data))                            # (the end-of-file member holds nothing)
            r = torch.tensor(np.array(ranges, np.int64), device=dev)
            check(turn, data, u[:-1], ranges, *eng.bgzf_read_ranges(t, len(image), coff, uoff, r))


def test_stream_teardown(eng):
    """nxz_stream_destroy gives the stream's scratch back and drops its entry; a new stream starts from nothing"""
    caller_tables(eng)
    inflate_check(eng, 130, 5)
    eng.torch.cuda.synchronize(eng.dev)
    old = eng.stream_handle.__self__
    old.destroy()
    new = OnStream(eng)
    try:
        caller_tables(eng)
        inflate_check(eng, 2, 6)
    finally:
        eng.torch.cuda.synchronize(eng.dev)
        new.destroy()
