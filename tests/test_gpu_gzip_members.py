"""GPU tests of the multi-member gzip calls (include/nxz_engine.h: nxz_batch_gzip_members_size / _decode; the index kernel and the
decode's plumbing in power-gzip_amd/csrc/nxz_gzip_members.hip).  Expected records and summaries come from the Python model
(tests/gzip_members_model.py), decoded bytes from zlib -- never from the engine."""
import ctypes as C
import importlib
import random
import threading

import numpy as np
import pytest

import framing as F
import gzip_members_model as M

pytestmark = pytest.mark.gpu
pkg = importlib.import_module("power-gzip_amd")
MDT, SDT = pkg.GZIP_MEMBER_DTYPE, pkg.GZIP_STREAM_DTYPE
POISON, GUARD = 0xEE, 32


@pytest.fixture(scope="module")
def eng():
    e = pkg.Engine(0)
    yield e
    e.close()


def place(eng, bufs, offs=None, fill=0xa5):
    """the buffers in one device tensor, buffer i at offs[i] bytes behind a 16-byte boundary; returns (tensor, addresses)"""
    import torch
    offs = offs or [0] * len(bufs)
    at, pos = [], 0
    for b, o in zip(bufs, offs):
        at.append(pos + o)
        pos += (o + len(b) + 15 + 16) & ~15
    host = np.full(max(pos, 16), fill, np.uint8)
    for b, a in zip(bufs, at):
        host[a:a + len(b)] = np.frombuffer(b, np.uint8)
    t = torch.from_numpy(host).to(eng.dev)
    return t, np.uint64(t.data_ptr()) + np.array(at, np.uint64)


class Batch:
    """jobs on the device: sources placed, a target with GUARD bytes of 0xAA on both sides of every job's dst_cap bytes"""

    def __init__(self, eng, bufs, cap, offs=None, dst_caps=None, resume=0, hist=0, dst_offs=None):
        import torch
        self.eng, self.bufs, self.cap, self.n = eng, bufs, cap, len(bufs)
        self.model = [M.walk(b, cap, r, h) for b, r, h in zip(bufs, np.broadcast_to(resume, self.n), np.broadcast_to(hist, self.n))]
        self.dst_caps = [s["out_len"] for s, _, _ in self.model] if dst_caps is None else list(dst_caps)
        self.src, addrs = place(eng, bufs, offs)
        dst_offs = dst_offs or [0] * self.n
        self.dat, pos = [], 0
        for c, o in zip(self.dst_caps, dst_offs):
            self.dat.append(pos + GUARD + o)
            pos += (GUARD + o + c + GUARD + 15) & ~15
        self.dst = torch.full((max(pos, 16),), 0xAA, dtype=torch.uint8, device=eng.dev)
        j = np.zeros(self.n, pkg.JOB_DTYPE)
        j["src"], j["src_len"], j["in_adler"] = addrs, [len(b) for b in bufs], 1
        j["dst"] = np.uint64(self.dst.data_ptr()) + np.array(self.dat, np.uint64)
        j["dst_cap"], j["resume"], j["hist_len"] = self.dst_caps, resume, hist
        self.jobs_host = j
        self.jobs = eng.to_device(j)
        self.members = torch.full((self.n * cap * MDT.itemsize,), POISON, dtype=torch.uint8, device=eng.dev)
        self.streams = torch.full((self.n * SDT.itemsize,), POISON, dtype=torch.uint8, device=eng.dev)

    def host(self):
        self.eng.torch.cuda.synchronize(self.eng.dev)
        return self.members.cpu().numpy().view(MDT).reshape(self.n, self.cap), self.streams.cpu().numpy().view(SDT)

    def size(self):
        self.eng.gzip_members_size(self.jobs, self.n, self.cap, self.members, self.streams)
        m, s = self.host()
        poison = np.frombuffer(bytes([POISON]) * MDT.itemsize, MDT)[0]
        for i, (ws, wrecs, _) in enumerate(self.model):
            assert [int(s[k][i]) for k in M.STREAM_FIELDS] == [ws[k] for k in M.STREAM_FIELDS], (i, s[i], ws)
            for k, w in enumerate(wrecs):
                assert [int(m[i, k][f]) for f in M.MEMBER_FIELDS] == [w[f] for f in M.MEMBER_FIELDS], (i, k, m[i, k], w)
            assert (m[i, len(wrecs):] == poison).all(), i        # slots behind the stored records are nobody's
            if ws["status"] != M.GZS_MEMBER_FAILED:
                assert int(s["cc"][i]) == 0, i
            elif ws["failed"] < self.cap and wrecs[-1]["status"] == F.DEFLATE:
                assert int(s["cc"][i]) not in (0, 3), i          # the raw decoder's code
        assert bool((self.dst == 0xAA).all())                    # the size pass writes nothing but the two arrays
        return m, s

    def decode(self, total=None, edit=None):
        """the decode on what size() left (edit: (job, slot, field, value) written into a record first); everything held against the model"""
        m0, s0 = self.host()
        model = [(dict(s), [dict(r) for r in recs], outs) for s, recs, outs in self.model]
        if edit is not None:
            i, k, field, value = edit
            m0[i, k][field] = value
            self.members.copy_(self.eng.torch.from_numpy(m0.view(np.uint8).reshape(-1).copy()))
            model[i][1][k][field] = value
        self.eng.gzip_members_decode(self.jobs, self.n, self.cap, self.members, self.streams, total)
        m, s = self.host()
        out = self.dst.cpu().numpy()
        want = np.full(out.shape, 0xAA, np.uint8)
        for i, (ws, wrecs, outs) in enumerate(model):
            ds, drecs, written = M.decode(self.bufs[i], ws, wrecs, outs, self.cap, self.dst_caps[i])
            assert [int(s[k][i]) for k in M.STREAM_FIELDS] == [ds[k] for k in M.STREAM_FIELDS], (i, s[i], ds)
            for k, w in enumerate(drecs):
                assert [int(m[i, k][f]) for f in M.MEMBER_FIELDS] == [w[f] for f in M.MEMBER_FIELDS], (i, k, m[i, k], w)
            for uoff, data in written:
                a = self.dat[i] + uoff
                want[a:a + len(data)] = np.frombuffer(data, np.uint8)
        bad = np.nonzero(out != want)[0]
        assert bad.size == 0, ("target differs at", bad[:8])
        return m, s

    def plain(self, i):
        out = self.dst.cpu().numpy()
        return out[self.dat[i]:self.dat[i] + self.dst_caps[i]].tobytes()


def series(seed, count, first=0, sizes=None):
    rnd = random.Random(seed)
    return [M.mixed_member(rnd, first + k, None if sizes is None else sizes[k]) for k in range(count)]


def test_member_counts(eng):
    ms = series(1, 17)
    bufs = [ms[1], b"".join(ms[:2]), b"".join(ms[2:5]), b"".join(ms), M.gz(b""), M.gz(b"") * 3]
    assert len(bufs[4]) == 20
    b = Batch(eng, bufs, 17, offs=[0, 5, 9, 14, 3, 0])
    m, s = b.size()
    assert [int(x) for x in s["members"]] == [1, 2, 3, 17, 1, 3]
    b.decode()
    for i, src in enumerate(bufs):
        assert b.plain(i) == M.plain(src)[0], i
    # a one-member job: what the framed size query says of it
    res, fr = eng.decompress_size_framed(pkg.FMT_GZIP, b.jobs, 1)
    r, f = eng.results_to_host(res), eng.frames_to_host(fr)
    assert int(f["status"][0]) == F.OK
    assert (int(m[0, 0]["hdr_len"]), int(m[0, 0]["check"]), int(m[0, 0]["isize"]), int(m[0, 0]["clen"])) == \
        (int(f["hdr_len"][0]), int(f["check"][0]), int(r["tpbc"][0]), int(f["end"][0]))


def test_alignment(eng):
    """src at 0..3 bytes behind a 16-byte boundary; member sizes such that the later members start at every residue mod 4"""
    rnd = random.Random(2)
    ms, k = [], 0
    while len(ms) < 12:                                      # sizes 4q, 4q + 1, 4q + 2, 4q + 3 in turn: starts at 0, 0, 1, 3, 2, ...
        c = M.mixed_member(rnd, k, rnd.randrange(1, 700))
        k += 1
        if len(c) % 4 == len(ms) % 4:
            ms.append(c)
    src = b"".join(ms)
    starts = set(sum(len(x) for x in ms[:i]) % 4 for i in range(len(ms)))
    assert starts == {0, 1, 2, 3}
    b = Batch(eng, [src] * 4, 12, offs=[0, 1, 2, 3], dst_offs=[0, 1, 2, 3])
    b.size()
    b.decode()
    assert all(b.plain(i) == M.plain(src)[0] for i in range(4))


def test_trailing_bytes(eng):
    ms = series(3, 3, first=1)
    three = b"".join(ms)
    bufs = [three + bytes(9), three + b"\0", three + b"\x1f\x8cgarbage!", three + b"\x1f", three + b"\x1f\x8b\x07\x00\x00", three + b"\x1f\x8b"]
    b = Batch(eng, bufs, 4, offs=[0, 3, 6, 9, 12, 15])
    m, s = b.size()
    for i in range(4):
        assert (int(s["status"][i]), int(s["members"][i]), int(s["consumed"][i])) == (pkg.GZS_OK, 3, len(three)), i
    assert (int(s["status"][4]), int(s["failed"][4]), int(m[4, 3]["status"])) == (pkg.GZS_MEMBER_FAILED, 3, F.BAD_METHOD)
    assert (int(s["status"][5]), int(s["failed"][5]), int(m[5, 3]["status"])) == (pkg.GZS_MEMBER_FAILED, 3, F.TRUNCATED)
    b.decode()
    want = M.plain(three)[0]
    assert all(b.plain(i)[:len(want)] == want for i in range(6))     # the members in front of a failed one are intact and decoded


def test_truncation(eng):
    rnd = random.Random(4)
    first = M.gz(M.payload(rnd, 1500), 6, **M.HEADERS[2])
    big = M.gz(M.payload(rnd, 2500), 6, **M.HEADERS[5])
    hl = F.parse(big, F.FMT_GZIP)["hdr_len"]
    cuts = [5, 11, 100, hl - 1, hl + 1, hl + (len(big) - hl) // 2, len(big) - 9, len(big) - 8, len(big) - 3, len(big) - 1]
    b = Batch(eng, [first + big[:c] for c in cuts], 4, offs=[i % 16 for i in range(len(cuts))])
    m, s = b.size()
    for i in range(len(cuts)):
        assert (int(s["status"][i]), int(s["members"][i]), int(s["failed"][i]), int(m[i, 1]["status"])) == (pkg.GZS_MEMBER_FAILED, 2, 1, F.TRUNCATED), i
    b.decode()
    assert all(b.plain(i) == M.plain(first)[0] for i in range(len(cuts)))


def test_wrong_trailer(eng):
    ms = series(5, 3, first=1)
    flip = lambda c, i: c[:i] + bytes([c[i] ^ 0x10]) + c[i + 1:]
    bad_isize = ms[0] + flip(ms[1], len(ms[1]) - 3) + ms[2]
    bad_crc = ms[0] + flip(ms[1], len(ms[1]) - 7) + ms[2]
    b = Batch(eng, [bad_isize, bad_crc], 4, offs=[7, 2])
    m, s = b.size()
    assert (int(s["status"][0]), int(s["failed"][0]), int(m[0, 1]["status"])) == (pkg.GZS_MEMBER_FAILED, 1, F.BAD_LENGTH)
    assert (int(s["status"][1]), int(s["members"][1]), int(s["failed"][1])) == (pkg.GZS_OK, 3, 3)       # the size pass cannot see the CRC
    m, s = b.decode()
    assert (int(s["status"][1]), int(s["failed"][1]), int(m[1, 1]["status"])) == (pkg.GZS_MEMBER_FAILED, 1, F.BAD_CHECK)
    assert int(m[1, 0]["status"]) == F.OK and int(m[1, 2]["status"]) == F.OK
    outs = [M.plain(x)[0] for x in ms]
    assert b.plain(1) == b"".join(outs)                      # members 0 and 2 (and the bytes of member 1) are there
    assert int(s["out_len"][1]) == len(outs[0]) + len(outs[2])


def test_member_cap(eng):
    five, other = b"".join(series(6, 5, first=1)), series(7, 1, first=1)[0]
    b = Batch(eng, [other, five, other], 2, offs=[1, 2, 3])  # (dst_cap: the model's out_len, the true size of all five)
    m, s = b.size()                                          # (the neighbours' second slots stay poison, their first the model's)
    assert (int(s["status"][1]), int(s["members"][1]), int(s["failed"][1])) == (pkg.GZS_MORE_MEMBERS, 5, 5)
    assert int(s["out_len"][1]) == len(M.plain(five)[0]) and int(s["consumed"][1]) == len(five)
    m, s = b.decode()
    two = b"".join(M.walk(five)[2][:2])
    assert int(s["status"][1]) == pkg.GZS_MORE_MEMBERS and int(s["out_len"][1]) == len(two)
    assert b.plain(1)[:len(two)] == two and set(b.plain(1)[len(two):]) == {0xAA}


def test_short_target_and_stale_records(eng):
    src = b"".join(series(8, 3, first=1))
    need = M.walk(src)[0]["out_len"]
    b = Batch(eng, [src, src, src], 3, dst_caps=[need, need - 1, need], offs=[0, 5, 10])
    b.size()
    m, s = b.decode()
    assert [int(x) for x in s["status"]] == [pkg.GZS_OK, pkg.GZS_TARGET_SPACE, pkg.GZS_OK]
    assert int(s["out_len"][1]) == need                      # what the target lacks room for
    for edit in ((0, 2, "clen", len(src)), (2, 1, "uoff", need), (0, 1, "isize", need), (2, 0, "coff", 0xfffffff0), (0, 1, "status", F.BAD_CHECK)):
        b = Batch(eng, [src, src, src], 3, offs=[3, 6, 9])
        b.size()
        m, s = b.decode(edit=edit)
        want = [pkg.GZS_OK] * 3
        want[edit[0]] = pkg.GZS_INVALID
        assert [int(x) for x in s["status"]] == want, edit


def test_invalid_jobs(eng):
    src = b"".join(series(9, 2, first=1))
    b = Batch(eng, [src] * 4, 2, resume=np.array([0, 1, 0, 0x00e80000], np.uint32), hist=np.array([0, 0, 16, 0], np.uint32))
    m, s = b.size()
    assert [int(x) for x in s["status"]] == [pkg.GZS_OK] + [pkg.GZS_INVALID] * 3
    for i in (1, 2, 3):
        assert s[i].tolist() == (pkg.GZS_INVALID, 0, 0, 0, 0, 0, 0), i
    m, s = b.decode()
    assert [int(x) for x in s["status"]] == [pkg.GZS_OK] + [pkg.GZS_INVALID] * 3


def test_argument_checks(eng):
    src = M.gz(b"hello")
    b = Batch(eng, [src, src], 2)
    L, p = eng.L, lambda t: t.data_ptr()
    h = eng.stream_handle()
    assert L.nxz_batch_gzip_members_size(eng.ctx, None, 0, 2, None, None, h) == 0
    assert L.nxz_batch_gzip_members_decode(eng.ctx, None, 0, 2, None, None, 0, h) == 0
    assert L.nxz_batch_gzip_members_size(eng.ctx, p(b.jobs), 2, 0, p(b.members), p(b.streams), h) == -22
    assert L.nxz_batch_gzip_members_decode(eng.ctx, p(b.jobs), 2, 0, p(b.members), p(b.streams), 4, h) == -22
    assert L.nxz_batch_gzip_members_decode(eng.ctx, p(b.jobs), 2, 2, p(b.members), p(b.streams), 1, h) == -22
    for args in ((None, p(b.members), p(b.streams)), (p(b.jobs), None, p(b.streams)), (p(b.jobs), p(b.members), None)):
        assert L.nxz_batch_gzip_members_size(eng.ctx, args[0], 2, 2, args[1], args[2], h) == -22
        assert L.nxz_batch_gzip_members_decode(eng.ctx, args[0], 2, 2, args[1], args[2], 4, h) == -22
    assert L.nxz_batch_gzip_members_size(None, p(b.jobs), 2, 2, p(b.members), p(b.streams), h) == -22
    eng.torch.cuda.synchronize(eng.dev)
    assert bool((b.members == POISON).all()) and bool((b.streams == POISON).all())      # a refused call writes nothing
    b.size()
    b.decode(total=2)                                        # the tightest bound: a member a job


def wide_batch(seed, n=300):
    rnd = random.Random(seed)
    bufs = []
    for i in range(n):
        ms = [M.mixed_member(rnd, rnd.randrange(1000), rnd.randrange(0, 3001)) for _ in range(rnd.randrange(1, 9))]
        bufs.append(b"".join(ms) + (b"" if i % 7 else b"\0\0"))
    return bufs


def test_wide_batch(eng):
    """300 jobs of 1 to 8 members of 0 to 3000 bytes: the length ordering (from 128 jobs on), more jobs than one pass of the plan's
    threads' first lanes, total_members = n * member_cap: empty slots among the framed jobs"""
    bufs = wide_batch(10)
    rnd = random.Random(11)
    b = Batch(eng, bufs, 8, offs=[rnd.randrange(16) for _ in bufs], dst_offs=[rnd.randrange(16) for _ in bufs])
    m, s = b.size()
    assert set(int(x) for x in s["members"]) == set(range(1, 9)) and int(s["members"].sum()) < len(bufs) * 8
    b.decode(total=len(bufs) * 8)
    for i in (0, 7, 150, 299):
        assert b.plain(i) == M.plain(bufs[i])[0], i


def test_many_small_members(eng):
    """one job of 2000 members of about 100 bytes: the loop inside the kernel, and more members than the plan's workgroup has threads"""
    rnd = random.Random(12)
    ms = [M.mixed_member(rnd, 1 + k % 4 + 5 * (k % 6), rnd.randrange(60, 140)) for k in range(2000)]
    src = b"".join(ms)
    b = Batch(eng, [src, ms[0] + ms[1]], 2000, offs=[0, 1])
    m, s = b.size()
    assert int(s["members"][0]) == 2000 and int(s["status"][0]) == pkg.GZS_OK
    b.decode()
    assert b.plain(0) == M.plain(src)[0]


def test_two_pass_recipe_on_the_device(eng):
    """size with a small member_cap, read two numbers, size again, lay out, decode -- the layout with torch on the device"""
    import torch
    bufs = wide_batch(13, 100)
    n = len(bufs)
    src, addrs = place(eng, bufs, offs=[(5 * i) % 16 for i in range(n)])
    j = np.zeros(n, pkg.JOB_DTYPE)
    j["src"], j["src_len"], j["in_adler"] = addrs, [len(x) for x in bufs], 1
    jobs = eng.to_device(j)
    # pass 1: how many members, how many bytes
    _, st = eng.gzip_members_size(jobs, n, 1)
    s32 = st.view(torch.int32).view(n, 8)
    out_len = st.view(torch.int64).view(n, 4)[:, 2]
    slot = (out_len + 15) & ~15
    offs = torch.cumsum(slot, 0) - slot
    cap, total = int(s32[:, 1].max().item()), int((offs[-1] + slot[-1]).item())     # the two numbers the host reads
    assert cap == 8 and total >= sum(len(M.plain(x)[0]) for x in bufs)
    members, st = eng.gzip_members_size(jobs, n, cap)
    dst = torch.empty(max(total, 16), dtype=torch.uint8, device=eng.dev)
    j64 = jobs.view(torch.int64).view(n, 6)
    j64[:, 1] = offs + dst.data_ptr()
    j64[:, 3] = out_len                                     # dst_cap (in_crc = 0 above it)
    # pass 2
    eng.gzip_members_decode(jobs, n, cap, members, st)
    s = eng.results_to_host(st, SDT)
    assert (s["status"] == pkg.GZS_OK).all()
    out, o = dst.cpu().numpy(), offs.cpu().numpy()
    for i, x in enumerate(bufs):
        want = M.plain(x)[0]
        assert int(s["out_len"][i]) == len(want) and out[o[i]:o[i] + len(want)].tobytes() == want, i


def test_two_streams_give_the_same(eng):
    """the same batch on two streams at once: scratch and frame_use are per stream"""
    L = eng.L
    L.nxz_stream_create.restype = C.c_void_p
    L.nxz_stream_create.argtypes = [C.c_void_p]
    L.nxz_stream_destroy.argtypes = [C.c_void_p, C.c_void_p]
    bufs = wide_batch(14, 200)
    rnd = random.Random(15)
    offs = [rnd.randrange(16) for _ in bufs]
    work = [Batch(eng, bufs, 8, offs=offs) for _ in range(2)]
    eng.torch.cuda.synchronize(eng.dev)
    handles = [L.nxz_stream_create(eng.ctx) for _ in range(2)]
    assert all(handles)
    rcs = [None, None]

    def run(k):
        b, h = work[k], C.c_void_p(handles[k])
        rc = 0
        for _ in range(3):
            rc = rc or L.nxz_batch_gzip_members_size(eng.ctx, b.jobs.data_ptr(), b.n, b.cap, b.members.data_ptr(), b.streams.data_ptr(), h)
            rc = rc or L.nxz_batch_gzip_members_decode(eng.ctx, b.jobs.data_ptr(), b.n, b.cap, b.members.data_ptr(), b.streams.data_ptr(), b.n * b.cap, h)
        rcs[k] = rc or L.nxz_ctx_sync(eng.ctx, h)
    threads = [threading.Thread(target=run, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert rcs == [0, 0]
    got = [(b.host(), b.dst.cpu().numpy()) for b in work]
    assert (got[0][0][0] == got[1][0][0]).all() and (got[0][0][1] == got[1][0][1]).all() and (got[0][1] == got[1][1]).all()
    for i in (0, 99, 199):
        assert work[0].plain(i) == M.plain(bufs[i])[0] and int(got[0][0][1]["status"][i]) == pkg.GZS_OK, i
    for h in handles:
        L.nxz_stream_destroy(eng.ctx, C.c_void_p(h))
