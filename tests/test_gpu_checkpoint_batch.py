"""GPU tests of the batched range read (include/nxz_engine.h: nxz_batch_checkpoint_read_ranges; the kernels in
power-gzip_amd/csrc/nxz_checkpoint_batch.hip): ranges over all the rows of an index that nxz_batch_checkpoint_build wrote, in one
call.  The expected bytes are slices of the plain data the streams were made of with Python's zlib, never the engine's; the
single-stream readers are run beside it on the same ranges.  Small shapes at which each step can still go wrong: rows that are good,
failed and overflowed in one batch, an empty stream and a stream of one segment between longer ones (the flat index's empty members),
ranges in shuffled job order, chunks of two segments that straddle streams, a fine index, a stale row, a damaged segment."""
import bisect
import ctypes as C
import errno
import importlib
import os
import random
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
pkg = importlib.import_module("power-gzip_amd")
KNOBS = ("NXZ_INFLATE_LANES_MIN", "NXZ_INFLATE_CUT", "NXZ_INFLATE_WG", "NXZ_INFLATE_WG_MAX", "NXZ_WG_PMIN", "NXZ_INFLATE_ORDER",
         "NXZ_BGZF_CHUNK", "NXZ_STREAMS_CHUNK")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W = pkg.CHECKPOINT_WINDOW
STATE = pkg.CHECKPOINT_STATE_DTYPE
OK, OOB, DAMAGED, BAD_STREAM = pkg.RANGE_OK, pkg.RANGE_OUT_OF_BOUNDS, pkg.RANGE_DAMAGED, pkg.RANGE_BAD_STREAM
FMT_RAW = pkg.engine.FMT_RAW


@pytest.fixture(scope="module")
def eng():
    saved = {k: os.environ.pop(k, None) for k in KNOBS}
    e = pkg.Engine(0)
    yield e
    e.close()
    for k, v in saved.items():
        if v is not None:
            os.environ[k] = v


@pytest.fixture
def chunks_of_two(monkeypatch):
    monkeypatch.setenv("NXZ_BGZF_CHUNK", "2")


def z(data, wbits, level=6, mem=8, strategy=zlib.Z_DEFAULT_STRATEGY):
    c = zlib.compressobj(level, zlib.DEFLATED, wbits, mem, strategy)
    return c.compress(data) + c.flush()


def text(n):
    a = open(os.path.join(ROOT, "tests", "golden", "alice29.txt"), "rb").read()
    return (a * (n // len(a) + 1))[:n]


class Indexed:
    """streams on the device at odd addresses, indexed by nxz_batch_checkpoint_build; plain[i] None: no row to read through"""

    def __init__(self, eng, fmt, streams, plain, span, cp_cap, state):
        import torch
        self.eng, self.fmt, self.streams_b, self.plain, self.cp_cap, self.n = eng, fmt, streams, plain, cp_cap, len(streams)
        self.at, pos = [], 0
        for i, st in enumerate(streams):                                  # src at any alignment: 16 k + 1, + 2, ...
            pos = ((pos + 15) & ~15) + (i + 1) % 16
            self.at.append(pos)
            pos += len(st)
        hs = np.zeros(pos + 16, np.uint8)
        for st, a in zip(streams, self.at):
            hs[a:a + len(st)] = np.frombuffer(st, np.uint8)
        self.src = torch.from_numpy(hs).to(eng.dev)
        j = np.zeros(self.n, pkg.JOB_DTYPE)
        for i in range(self.n):
            j[i]["src"] = self.src.data_ptr() + self.at[i]
            j[i]["src_len"] = len(streams[i])
            j[i]["in_adler"] = 1
        self.jobs = eng.to_device(j)
        rc, self.cbit, self.uoff, self.state, self.windows, self.streams = eng.checkpoint_build(fmt, self.jobs, self.n, span, cp_cap, state=state)
        assert rc == 0
        self.st = eng.results_to_host(self.streams, pkg.CHECKPOINT_STREAM_DTYPE)[:self.n].copy()
        self.h_uoff = self.uoff.cpu().numpy()
        self.h_cbit = self.cbit.cpu().numpy()

    def read(self, ranges, state="own", **over):
        """-> (rc, offsets, status, out_len, decoded, bytes) on the host"""
        import torch
        eng = self.eng
        q = np.zeros(len(ranges), pkg.BATCH_RANGE_DTYPE)
        for r, (job, b, e) in enumerate(ranges):
            q[r] = (job, 0, b, e)
        a = dict(jobs=self.jobs, n_jobs=self.n, cp_cap=self.cp_cap, cbit=self.cbit, uoff=self.uoff, state=self.state if state == "own" else state,
                 windows=self.windows, streams=self.streams)
        a.update(over)
        rc, offs, status, out_len, decoded, dst = eng.checkpoint_read_ranges_batch(a["jobs"], a["n_jobs"], a["cp_cap"], a["cbit"], a["uoff"], a["state"],
                                                                                   a["windows"], a["streams"], eng.to_device(q))
        torch.cuda.synchronize(eng.dev)
        return rc, offs.cpu().numpy(), status.cpu().numpy(), out_len, decoded, dst.cpu().numpy()

    def expect(self, ranges, bad_rows=()):
        """per range: (status, bytes) from the plain data alone"""
        out = []
        for job, b, e in ranges:
            p = self.plain[job] if job < self.n else None
            if p is None or job in bad_rows:
                out.append((BAD_STREAM, b""))
            elif b > e or e > len(p):
                out.append((OOB, b""))
            else:
                out.append((OK, p[b:e]))
        return out

    def touched(self, ranges, bad_rows=()):
        """the distinct segments the OK ranges touch, from the index's own uoff: the upper-bound rule"""
        seg = set()
        for (job, b, e), (st, _) in zip(ranges, self.expect(ranges, bad_rows)):
            if st == OK and b < e:
                u = self.h_uoff[job, :int(self.st[job]["count"])].tolist()
                seg |= {(job, k) for k in range(bisect.bisect_right(u, b) - 1, bisect.bisect_right(u, e - 1))}
        return seg

    def check(self, ranges, got, bad_rows=(), damaged=()):
        """damaged: segments (job, k) that do not decode: the ranges that touch one read zeros"""
        rc, offs, status, out_len, decoded, data = got
        assert rc == 0
        want = self.expect(ranges, bad_rows)
        pos = 0
        for r, ((job, b, e), (st, by)) in enumerate(zip(ranges, want)):
            hit = bool(self.touched([ranges[r]], bad_rows) & set(damaged))
            assert status[r] == (DAMAGED if hit else st), (r, job, b, e, status[r])
            assert offs[r] == pos, (r, job, b, e)
            assert data[pos:pos + len(by)].tobytes() == (bytes(len(by)) if hit else by), (r, job, b, e)
            pos += len(by)
        assert offs[len(ranges)] == pos == out_len
        assert decoded == len(self.touched(ranges, bad_rows))

    def single(self, job, ranges, fine):
        """the same ranges of one job through the single-stream reader -> (rc, status, [bytes])"""
        import torch
        eng, cnt, length = self.eng, int(self.st[job]["count"]), len(self.streams_b[job])
        src = self.src[self.at[job]:self.at[job] + length].clone()
        r = torch.tensor(np.array([(b, e) for _, b, e in ranges], np.int64).reshape(-1, 2), device=eng.dev)
        n = min(cnt, self.cp_cap) + 1
        cb, uo, wi = self.cbit[job, :n].contiguous(), self.uoff[job, :n].contiguous(), self.windows[job, :n - 1].contiguous()
        if fine:
            got = eng.checkpoint_read_ranges_fine(src, length, cb, uo, self.state[job, :n * STATE.itemsize].contiguous(), wi, r)
        else:
            got = eng.checkpoint_read_ranges(src, length, cb, uo, wi, r)
        torch.cuda.synchronize(eng.dev)
        rc, offs, status, out_len, decoded, dst = got
        offs, data = offs.cpu().numpy(), dst.cpu().numpy()
        return rc, status.cpu().numpy(), [data[offs[i]:offs[i + 1]].tobytes() for i in range(len(ranges))]


# ---- 1. the mixed batch ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mixed(eng):
    long_text, more_text = text(200 << 10), text(400 << 10)
    a = z(long_text, 15, 6, 6)                                            # (memLevel 6: a block every 20 KiB or so, a checkpoint every other block)
    streams = [a, z(text(70 << 10), 31), z(b"one short block", 15), z(b"", 15), a[:len(a) // 2], z(more_text, 15, 6, 6)]
    plain = [long_text, text(70 << 10), b"one short block", b"", None, None]
    m = Indexed(eng, pkg.FMT_AUTO, streams, plain, 32768, 8, state=False)
    return m


def mixed_ranges(m):
    n0, n1 = len(m.plain[0]), len(m.plain[1])
    u0 = m.h_uoff[0].tolist()
    r = [(0, u0[1] + 10, u0[1] + 4106), (0, u0[1] + 5000, u0[1] + 5100),                # inside one segment, twice in the same segment
         (0, u0[2] - 100, u0[2] + 100), (0, u0[1] - 1, u0[4] + 1), (0, 0, n0), (0, n0 - 1, n0), (0, 0, 1), (0, u0[3], u0[4]),
         (0, 77, 77), (0, n0, n0), (0, 9, 8), (0, n0 - 5, n0 + 1), (0, n0 + 1, n0 + 1), (0, u0[4] + 3, n0),
         (1, 0, n1), (1, 40000, 44096), (1, 100, 100), (1, 0, n1 + 1), (1, n1 - 4096, n1), (1, 34000, 36000),
         (2, 0, 15), (2, 3, 9), (2, 0, 16), (2, 15, 15), (2, 16, 15),
         (3, 0, 0), (3, 0, 1), (3, 1, 1),
         (4, 0, 1), (4, 0, 0), (4, 5, 4),
         (5, 0, 4096), (5, 0, 0), (5, 100000, 100001),
         (6, 0, 0), (6, 0, 10), (0xffffffff, 0, 0),
         (0, 123, 4219), (1, 1, 2), (2, 14, 15), (0, u0[2], u0[2] + 1)]
    random.Random(5).shuffle(r)
    return r


def test_the_mixed_batch_is_what_it_should_be(mixed):
    st = mixed.st
    assert [int(s["status"]) for s in st] == [pkg.CPS_OK, pkg.CPS_OK, pkg.CPS_OK, pkg.CPS_OK, pkg.CPS_STREAM_FAILED, pkg.CPS_MORE]
    assert int(st[0]["count"]) >= 5 and mixed.h_uoff[0, 3] >= W and int(st[2]["count"]) == 1 and int(st[3]["out_len"]) == 0 and int(st[5]["count"]) > 8
    assert [int(s["out_len"]) for s in st[:4]] == [200 << 10, 70 << 10, 15, 0]
    r = mixed_ranges(mixed)
    assert len(r) >= 40 and len({j for j, _, _ in r[:8]}) >= 3             # shuffled job order


def test_mixed_batch_statuses_offsets_bytes_and_decoded(mixed):
    r = mixed_ranges(mixed)
    got = mixed.read(r)
    mixed.check(r, got)
    st = got[2].tolist()
    assert {OK, OOB, BAD_STREAM} == set(st) and st.count(BAD_STREAM) == 9 and got[4] == int(mixed.st[0]["count"]) + int(mixed.st[1]["count"]) + 1


def test_mixed_batch_equals_the_single_stream_reader(mixed):
    r = mixed_ranges(mixed)
    rc, offs, status, out_len, decoded, data = mixed.read(r)
    assert rc == 0
    for job in range(7):
        mine = [i for i, q in enumerate(r) if q[0] == job]
        assert mine
        if job < 4:
            rc1, st1, by1 = mixed.single(job, [r[i] for i in mine], fine=False)
            assert rc1 == 0
            for i, s, b in zip(mine, st1, by1):
                assert status[i] == s and data[offs[i]:offs[i + 1]].tobytes() == b, (job, r[i])
        else:
            if job == 4:                                                  # count 0: the single-stream call refuses the index
                assert mixed.single(job, [r[i] for i in mine], fine=False)[0] == -errno.EINVAL
            # (the overflowed row has no sentinel and job == n_jobs has no row: there is nothing to call the single reader with)
            assert all(status[i] == BAD_STREAM and offs[i] == offs[i + 1] for i in mine), job


def test_two_raw_streams(eng):
    a, b = text(90 << 10), text(150 << 10)[::-1]
    m = Indexed(eng, FMT_RAW, [z(a, -15, 6, 6), z(b, -15, 1, 6)], [a, b], 32768, 8, state=False)
    assert [int(s["status"]) for s in m.st] == [pkg.CPS_OK, pkg.CPS_OK] and int(m.st[1]["count"]) >= 2
    r = [(1, 0, len(b)), (0, 5, 40000), (1, 70000, 70100), (0, len(a) - 1, len(a)), (2, 0, 1), (1, len(b), len(b) + 1), (0, 0, 0)]
    m.check(r, m.read(r))


# ---- 2. chunks straddle streams ----------------------------------------------------------------------------------------------------
def test_chunks_of_two_segments_give_the_same_output(mixed, chunks_of_two):
    r = mixed_ranges(mixed)
    assert os.environ["NXZ_BGZF_CHUNK"] == "2"
    chunked = mixed.read(r)
    mixed.check(r, chunked)
    del os.environ["NXZ_BGZF_CHUNK"]
    whole = mixed.read(r)
    assert chunked[0] == whole[0] == 0 and chunked[3:5] == whole[3:5] and chunked[4] > 2 * 3          # several chunks, some across two streams
    for a, b in zip(chunked[1:3] + chunked[5:], whole[1:3] + whole[5:]):
        assert np.array_equal(a, b)


# ---- 3. the fine index -------------------------------------------------------------------------------------------------------------
def fine_streams():
    p = [text(100 << 10), text(150 << 10), text(200 << 10)]
    return [z(p[0], 15, 6, 9, zlib.Z_FIXED), z(p[1], 15, 0), z(p[2], 15, 6)], p        # (memLevel 9: the fixed stream is ONE block)


@pytest.fixture(scope="module")
def fine(eng):
    s, p = fine_streams()
    return Indexed(eng, pkg.FMT_AUTO, s, p, 4096, 64, state=True)


def fine_ranges(m):
    rnd = random.Random(9)
    r = [(j, 0, len(m.plain[j])) for j in range(3)]
    for j in range(3):
        n = len(m.plain[j])
        r += [(j, b, min(n, b + rnd.choice([1, 300, 5000, 70000]))) for b in (rnd.randrange(n) for _ in range(8))]
        u = m.h_uoff[j]
        r += [(j, int(u[k]) - 1, int(u[k]) + 1) for k in (1, int(m.st[j]["count"]) - 1) if 1 <= k < int(m.st[j]["count"])]   # across a checkpoint
    rnd.shuffle(r)
    return r


def test_fine_index_reads_inside_blocks(fine):
    sta = fine.state.cpu().numpy()
    kinds = [{(int(s["resume"]) >> 16) & 0xe for s in sta[j].view(STATE)[:int(fine.st[j]["count"])]} for j in range(3)]
    assert [int(s["status"]) for s in fine.st] == [pkg.CPS_OK] * 3 and all(24 <= int(s["count"]) <= 64 for s in fine.st)
    assert 0xa in kinds[0] and 0x8 in kinds[1] and 0xc in kinds[2]          # checkpoints inside fixed, stored and dynamic blocks
    r = fine_ranges(fine)
    got = fine.read(r)
    fine.check(r, got)
    for job in range(3):                                                  # ... and what the single-stream fine reader gives
        mine = [i for i, q in enumerate(r) if q[0] == job]
        rc1, st1, by1 = fine.single(job, [r[i] for i in mine], fine=True)
        assert rc1 == 0
        for i, s, b in zip(mine, st1, by1):
            assert got[2][i] == s and got[5][got[1][i]:got[1][i + 1]].tobytes() == b


def test_a_coarse_index_of_the_same_jobs_without_states(eng):
    s, p = fine_streams()
    m = Indexed(eng, pkg.FMT_AUTO, s, p, 4096, 64, state=False)
    assert m.state is None and [int(x["status"]) for x in m.st] == [pkg.CPS_OK] * 3 and int(m.st[0]["count"]) == 1
    r = fine_ranges(m)
    got = m.read(r, state=None)
    m.check(r, got)
    zeros = eng.torch.zeros((3, 65 * STATE.itemsize), dtype=eng.torch.uint8, device=eng.dev)
    same = m.read(r, state=zeros)                                         # state == NULL reads what state all zero reads
    assert got[3:5] == same[3:5] and all(np.array_equal(a, b) for a, b in zip(got[1:3] + got[5:], same[1:3] + same[5:]))


# ---- 4. a stale row is that row's problem ------------------------------------------------------------------------------------------
def test_a_row_whose_cbit_does_not_increase(fine):
    r = fine_ranges(fine)
    cb = fine.cbit.clone()
    cb[1, 7] = cb[1, 6]
    fine.check(r, fine.read(r, cbit=cb), bad_rows=(1,))
    cb = fine.cbit.clone()
    cb[0, int(fine.st[0]["count"])] = 8 * len(fine.streams_b[0]) + 1       # the sentinel behind the source
    fine.check(r, fine.read(r, cbit=cb), bad_rows=(0,))


def test_a_row_whose_table_ends_behind_its_checkpoint(fine):
    r = fine_ranges(fine)
    sta = fine.state.cpu().numpy().copy()
    row = sta[2].view(STATE)
    k = next(k for k in range(1, int(fine.st[2]["count"])) if (int(row[k]["resume"]) >> 16) & 0xe == 0xc)
    row[k]["tbit"] = int(fine.h_cbit[2, k]) - int(row[k]["dhtlen"]) + 1     # tbit + dhtlen > cbit
    got = fine.read(r, state=fine.eng.torch.from_numpy(sta).to(fine.eng.dev))
    fine.check(r, got, bad_rows=(2,))
    assert got[2].tolist().count(BAD_STREAM) == sum(1 for q in r if q[0] == 2) >= 10


# ---- 5. damage ---------------------------------------------------------------------------------------------------------------------
def test_a_damaged_segment_costs_its_ranges_only(mixed):
    import torch
    r = mixed_ranges(mixed)
    cb = mixed.h_cbit[0]
    lo, hi = (int(cb[2]) + 7) // 8 + 1, int(cb[3]) // 8 - 1                 # bytes that are segment 2's alone
    stream = mixed.streams_b[0]
    for at in range(lo + 200, hi):                                        # a flip that zlib cannot decode: no flip without effect
        bad = bytearray(stream)
        bad[at] ^= 0xff
        try:
            zlib.decompressobj(-15).decompress(bytes(bad[2:-4]))
        except zlib.error:
            break
    else:
        raise AssertionError("no byte whose flip breaks the stream")
    with pytest.raises(zlib.error):
        zlib.decompress(bytes(bad))
    keep = mixed.src[mixed.at[0] + at].clone()
    mixed.src[mixed.at[0] + at] = int(bad[at])
    try:
        got = mixed.read(r)
    finally:
        mixed.src[mixed.at[0] + at] = keep
        torch.cuda.synchronize(mixed.eng.dev)
    mixed.check(r, got, damaged=((0, 2),))
    hit = [i for i, q in enumerate(r) if mixed.touched([q]) & {(0, 2)}]
    assert len(hit) >= 4 and all(got[2][i] == DAMAGED for i in hit) and got[2].tolist().count(DAMAGED) == len(hit)
    mixed.check(r, mixed.read(r))                                         # the source is whole again


# ---- 6. sizing and refusals --------------------------------------------------------------------------------------------------------
def test_sizing_and_refusals(eng, mixed):
    import torch
    t = torch
    m, L, h = mixed, eng.L, eng.stream_handle()
    r = mixed_ranges(m)
    n = len(r)
    q = np.zeros(n, pkg.BATCH_RANGE_DTYPE)
    for i, (job, b, e) in enumerate(r):
        q[i] = (job, 0, b, e)
    ranges = eng.to_device(q)
    offsets = t.full((n + 1,), -1, dtype=t.int64, device=eng.dev)
    status = t.full((n,), -1, dtype=t.int32, device=eng.dev)
    out_len, decoded = C.c_uint64(7), C.c_uint64(7)
    good = dict(ctx=eng.ctx, jobs=m.jobs.data_ptr(), n_jobs=m.n, cp_cap=m.cp_cap, cbit=m.cbit.data_ptr(), uoff=m.uoff.data_ptr(), state=None,
                windows=m.windows.data_ptr(), streams=m.streams.data_ptr(), ranges=ranges.data_ptr(), n=n, dst=None, dst_cap=0,
                offsets=offsets.data_ptr(), status=status.data_ptr())

    def call(**over):
        a = dict(good, **over)
        return L.nxz_batch_checkpoint_read_ranges(a["ctx"], a["jobs"], a["n_jobs"], a["cp_cap"], a["cbit"], a["uoff"], a["state"], a["windows"], a["streams"],
                                                  a["ranges"], a["n"], a["dst"], a["dst_cap"], a["offsets"], a["status"], C.byref(out_len), C.byref(decoded), h)
    # dst == NULL: the size, with offsets and status written
    want = m.expect(r)
    total = sum(len(b) for _, b in want)
    assert call() == -errno.E2BIG and out_len.value == total and decoded.value == 0
    t.cuda.synchronize(eng.dev)
    assert status.cpu().tolist() == [s for s, _ in want] and offsets.cpu().tolist() == list(np.cumsum([0] + [len(b) for _, b in want]))
    dst = t.zeros(total, dtype=t.uint8, device=eng.dev)
    assert call(dst=dst.data_ptr(), dst_cap=total - 1) == -errno.E2BIG and out_len.value == total
    assert call(dst=dst.data_ptr(), dst_cap=total) == 0 and out_len.value == total and decoded.value == len(m.touched(r))
    # nothing to read; nothing to read through
    assert call(n=0) == 0 and out_len.value == 0 and decoded.value == 0
    assert call(n=0, ranges=None, status=None) == 0
    status.fill_(-1)
    assert call(n_jobs=0, jobs=None) == 0 and out_len.value == 0
    t.cuda.synchronize(eng.dev)
    assert status.cpu().tolist() == [BAD_STREAM] * n and offsets.cpu().tolist() == [0] * (n + 1)
    # -EINVAL
    for bad in (dict(ctx=None), dict(cbit=None), dict(uoff=None), dict(windows=None), dict(streams=None), dict(offsets=None), dict(jobs=None),
                dict(cp_cap=0), dict(n_jobs=1 << 31), dict(n=1 << 31), dict(n_jobs=1 << 16, cp_cap=(1 << 16) - 1), dict(n_jobs=2, cp_cap=0xffffffff),
                dict(ranges=None), dict(status=None)):
        assert call(**bad) == -errno.EINVAL, bad
    assert call(dst=dst.data_ptr(), dst_cap=total) == 0
