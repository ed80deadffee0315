"""GPU tests of the fine checkpoint calls (include/nxz_engine.h: nxz_batch_checkpoint_index_fine, nxz_checkpoint_read_ranges_fine;
kernels in power-gzip_amd/csrc/nxz_checkpoint_fine.hip): ONE batch of raw, zlib and gzip streams of 100-250 KiB of plain bytes each
(tests/checkpoint_fine_model.streams() and one the engine wrote itself) indexed with spans of 258, 1000, 4096, 65536 and one above
every out_len against the model (tests/checkpoint_fine_model.py), then ranges read through index, states and windows alone against
slices of the plain bytes, and a chain of suspended decompress jobs as an independent check of where the checkpoints stand."""
import bisect
import errno
import importlib
import os
import random

import numpy as np
import pytest

import checkpoint_fine_model as F
import checkpoint_model as M

pytestmark = pytest.mark.gpu
pkg = importlib.import_module("power-gzip_amd")
KNOBS = ("NXZ_INFLATE_LANES_MIN", "NXZ_INFLATE_CUT", "NXZ_INFLATE_WG", "NXZ_INFLATE_WG_MAX", "NXZ_WG_PMIN", "NXZ_INFLATE_ORDER",
         "NXZ_BGZF_CHUNK", "NXZ_STREAMS_CHUNK")
W = F.WINDOW
PATTERN = 0xA5
SPANS = (258, 1000, 4096, 65536, 1 << 20)
STATE = pkg.CHECKPOINT_STATE_DTYPE


@pytest.fixture(scope="module")
def eng():
    saved = {k: os.environ.pop(k, None) for k in KNOBS}
    e = pkg.Engine(0)
    yield e
    e.close()
    for k, v in saved.items():
        if v is not None:
            os.environ[k] = v


def engine_stream(eng, data):
    """data as nxz_batch_deflate_streams writes it: a zlib stream of 64 KiB blocks"""
    import torch
    buf = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).to(eng.dev)
    out, offsets, results = eng.deflate_streams(pkg.FC_COMPRESS_DHTGEN, pkg.FMT_ZLIB, [buf])
    r = eng.results_to_host(results, pkg.engine.STREAM_RESULT_DTYPE)[0]
    assert r["cc"] == 0
    return out[:int(r["out_len"])].cpu().numpy().tobytes()


class Batch:
    """the streams on the device, 16-byte aligned, and per stream a target slot that holds its decoded output"""

    def __init__(self, eng, pick=None, parent=None):
        import torch
        if parent is not None:                                            # a part of the batch as a batch of its own
            self.__dict__.update(parent.__dict__)
            for f in ("names", "fmt", "stream", "plain", "sat", "dat", "cap"):
                setattr(self, f, [getattr(parent, f)[i] for i in pick])
            self.model = {span: [parent.model[span][i] for i in pick] for span in SPANS}
            self.n = len(pick)
            return
        s = list(F.streams())
        text = s[0][3]
        s.insert(9, ("engine", F.FMT_ZLIB, engine_stream(eng, text), text))
        self.names, self.fmt, self.stream, self.plain = ([x[k] for x in s] for k in range(4))
        self.n, self.eng = len(s), eng
        self.model = {span: [F.index(st, f, span) for st, f in zip(self.stream, self.fmt)] for span in SPANS}
        for span in SPANS:
            for i, m in enumerate(self.model[span]):
                assert (m is None) == (self.plain[i] is None) and (m is None or m["out_len"] == len(self.plain[i])), self.names[i]
        self.sat, pos = [], 0
        for st in self.stream:
            self.sat.append(pos)
            pos += (len(st) + 31) & ~15
        hs = np.zeros(pos + 16, np.uint8)
        for st, a in zip(self.stream, self.sat):
            hs[a:a + len(st)] = np.frombuffer(st, np.uint8)
        self.src = torch.from_numpy(hs).to(eng.dev)
        self.cap = [len(p) if p is not None else 4096 for p in self.plain]
        self.dat, pos = [], 0
        for c in self.cap:
            self.dat.append(pos)
            pos += (c + 31) & ~15
        hd = np.full(pos + 16, PATTERN, np.uint8)
        for p, a in zip(self.plain, self.dat):
            if p:
                hd[a:a + len(p)] = np.frombuffer(p, np.uint8)
        self.dst_host = hd
        self.dst = torch.from_numpy(hd).to(eng.dev)

    def jobs(self, dst=None, repeat=1, **fields):
        j = np.zeros(self.n, pkg.JOB_DTYPE)
        for i in range(self.n):
            j[i]["src"] = self.src.data_ptr() + self.sat[i]
            j[i]["src_len"] = len(self.stream[i])
            j[i]["dst"] = 0 if dst is None else dst.data_ptr() + self.dat[i]
            j[i]["dst_cap"] = self.cap[i]
            j[i]["in_adler"] = 1
        for k, v in fields.items():
            j[k] = v
        return self.eng.to_device(np.tile(j, repeat))

    def index(self, fmt, span, cp_cap, windows=False, dst=None, repeat=1, **fields):
        import torch
        eng, n = self.eng, self.n * repeat
        if windows:
            windows = torch.full((n, cp_cap, W), PATTERN, dtype=torch.uint8, device=eng.dev)
        cbit = torch.full((n, cp_cap + 1), -1, dtype=torch.int64, device=eng.dev)
        uoff = torch.full((n, cp_cap + 1), -1, dtype=torch.int64, device=eng.dev)
        state = torch.full((n, (cp_cap + 1) * STATE.itemsize), PATTERN, dtype=torch.uint8, device=eng.dev)
        rc, cbit, uoff, state, windows, streams = eng.checkpoint_index_fine(fmt, self.jobs(dst, repeat, **fields), n, span, cp_cap, windows, cbit, uoff, state)
        assert rc == 0
        st = eng.results_to_host(streams, pkg.CHECKPOINT_STREAM_DTYPE)[:n]
        return cbit, uoff, state, windows, st


@pytest.fixture(scope="module")
def batch(eng):
    return Batch(eng)


@pytest.fixture(scope="module")
def halves(batch):
    """the raw streams and the framed ones as batches of their own (raw streams have no header to tell them by)"""
    raw = [i for i in range(batch.n) if batch.fmt[i] == F.FMT_RAW]
    framed = [i for i in range(batch.n) if batch.fmt[i] != F.FMT_RAW]
    assert len(raw) == 4 and len(framed) == 9
    return ((Batch(None, raw, batch), pkg.engine.FMT_RAW), (Batch(None, framed, batch), pkg.FMT_AUTO))


def states_of(state_row):
    return [tuple(int(x) for x in s) for s in state_row.view(STATE)]


def check_positions(sub, span, cp_cap, cbit, uoff, state, st):
    """streams[], cbit, uoff and state against the model; entries behind what a stream stores still hold the fill"""
    cb, uo, sta = cbit.cpu().numpy(), uoff.cpu().numpy(), state.cpu().numpy()
    for i, m in enumerate(sub.model[span]):
        name, s = sub.names[i], st[i]
        if m is None:
            assert s["status"] == pkg.CPS_STREAM_FAILED and s["count"] == 0 and s["cc"] != 0 and s["out_len"] == 0, (name, s)
            assert (s["frame_status"], s["cc"] == 3) == ((pkg.FRAME_TRUNCATED, True) if name == "truncated" else (pkg.FRAME_DEFLATE, False)), (name, s)
            continue
        exp = pkg.CPS_MORE if m["count"] > cp_cap else pkg.CPS_OK
        assert (s["status"], s["count"], s["out_len"], s["cc"], s["frame_status"]) == (exp, m["count"], m["out_len"], 0, pkg.FRAME_OK), (name, span, s, m["count"])
        assert s["format"] == sub.fmt[i] and s["hdr_len"] == m["hdr_len"], (name, s)
        k = min(m["count"], cp_cap) + (0 if exp == pkg.CPS_MORE else 1)     # (with the sentinel, unless checkpoints were only counted)
        assert cb[i, :k].tolist() == m["cbit"][:k] and uo[i, :k].tolist() == m["uoff"][:k], (name, span)
        assert states_of(sta[i, :k * 16]) == (m["state"][:k] if exp == pkg.CPS_MORE else m["state"][:k - 1] + [(0, 0, 0)]), (name, span)
        assert (cb[i, k:] == -1).all() and (uo[i, k:] == -1).all() and (sta[i, k * 16:] == PATTERN).all(), (name, span)


def check_windows(sub, span, cp_cap, windows):
    w = windows.cpu().numpy()
    for i, m in enumerate(sub.model[span]):
        stored = min(m["count"], cp_cap) if m is not None else 0
        for k in range(stored):
            u = m["uoff"][k]
            n = min(u, W)
            assert w[i, k, :n].tobytes() == sub.plain[i][u - n:u] and (w[i, k, n:] == PATTERN).all(), (sub.names[i], k)
        assert (w[i, stored:] == PATTERN).all(), sub.names[i]


def test_the_batch_is_what_the_issue_asks_for(batch):
    assert batch.n == 13 and all(p is None or 100 << 10 <= len(p) <= 250 << 10 for p in batch.plain)
    assert batch.names == ["alice6_raw", "alice6_zlib", "alice6_gzip_fields", "alice1", "fixed_one_block", "rle_zeros", "stored", "mem9", "mem1",
                           "engine", "empty_final_block", "truncated", "bad_table"]
    m = dict(zip(batch.names, batch.model[1000]))
    sizes = np.diff(m["rle_zeros"]["uoff"])
    assert (sizes[1:-1] == 774).all() and all(m[n] is None for n in ("truncated", "bad_table"))
    assert all(mm is None or mm["count"] == 1 for mm in batch.model[1 << 20])


@pytest.mark.parametrize("span", SPANS)
def test_positions_states_and_windows_equal_the_model(halves, span):
    for sub, fmt in halves:
        cp_cap = max(m["count"] for m in sub.model[span] if m is not None) + 1
        windows = span >= 4096                                               # (below: hundreds of slots a stream; the copy is the coarse call's)
        cbit, uoff, state, wins, st = sub.index(fmt, span, cp_cap, windows=windows, dst=sub.dst)
        check_positions(sub, span, cp_cap, cbit, uoff, state, st)
        if windows:
            check_windows(sub, span, cp_cap, wins)


def test_the_one_block_stream_is_cut_where_the_coarse_index_cannot(eng, halves):
    sub, fmt = halves[0]
    i = sub.names.index("fixed_one_block")
    _, _, _, _, st = sub.index(fmt, 4096, 64)
    rc, _, _, _, streams = eng.checkpoint_index(fmt, sub.jobs(), sub.n, 4096, 64)
    coarse = eng.results_to_host(streams, pkg.CHECKPOINT_STREAM_DTYPE)
    assert rc == 0 and coarse[i]["status"] == pkg.CPS_OK and coarse[i]["count"] == 1
    assert st[i]["status"] == pkg.CPS_OK and st[i]["count"] == sub.model[4096][i]["count"] >= len(sub.plain[i]) // 4096


def test_a_small_cap_counts_on_and_no_windows_no_touch(halves, batch):
    import torch
    for sub, fmt in halves:
        cp_cap = sub.model[4096][0]["count"] - 1
        assert cp_cap >= 2
        cbit, uoff, state, wins, st = sub.index(fmt, 4096, cp_cap, windows=True, dst=sub.dst)
        assert st[0]["status"] == pkg.CPS_MORE and st[0]["count"] == cp_cap + 1
        check_positions(sub, 4096, cp_cap, cbit, uoff, state, st)
        check_windows(sub, 4096, cp_cap, wins)
        scratch = torch.full_like(batch.dst, PATTERN)
        cbit, uoff, state, wins, st = sub.index(fmt, 4096, 64, windows=False, dst=scratch)
        assert wins is None and bool((scratch == PATTERN).all())
        check_positions(sub, 4096, 64, cbit, uoff, state, st)
    assert torch.equal(batch.dst.cpu(), torch.from_numpy(batch.dst_host))


def test_refusals(eng, halves):
    sub, fmt = halves[1]
    for field, value in (("hist_len", 16), ("resume", 3 << 20)):
        v = np.zeros(sub.n, np.uint32)
        v[1] = value
        cbit, uoff, state, _, st = sub.index(fmt, 4096, 64, **{field: v})
        assert st[1]["status"] == pkg.CPS_INVALID and st[1]["count"] == 0 and st[1]["out_len"] == 0
        assert (cbit[1] == -1).all() and st[0]["status"] == pkg.CPS_OK and st[2]["status"] == pkg.CPS_OK
    jobs = sub.jobs()
    for args in ((fmt, jobs, sub.n, 257, 16), (fmt, jobs, sub.n, 0, 16), (fmt, jobs, sub.n, 4096, 0), (7, jobs, sub.n, 4096, 16)):
        assert eng.checkpoint_index_fine(*args)[0] == -errno.EINVAL
    assert eng.checkpoint_index_fine(fmt, jobs, sub.n, 258, 16)[0] == 0 and eng.checkpoint_index_fine(fmt, None, 0, 4096, 16)[0] == 0


def test_a_second_index_call_allocates_nothing(eng, halves):
    """130 jobs: the long ones first, the order in the stream's scratch -- which the second call finds as it is"""
    import torch
    sub, fmt = halves[1]
    first = sub.index(fmt, 65536, 8, repeat=15)
    torch.cuda.synchronize(eng.dev)
    jobs = sub.jobs(repeat=15)
    cbit, uoff, state, streams = first[0].clone().fill_(-1), first[1].clone().fill_(-1), first[2].clone().fill_(PATTERN), torch.zeros(sub.n * 15 * 32, dtype=torch.uint8, device=eng.dev)
    torch.cuda.synchronize(eng.dev)
    free0 = torch.cuda.mem_get_info(eng.dev)[0]
    rc = eng.checkpoint_index_fine(fmt, jobs, sub.n * 15, 65536, 8, False, cbit, uoff, state, streams)[0]
    torch.cuda.synchronize(eng.dev)
    assert rc == 0 and torch.cuda.mem_get_info(eng.dev)[0] == free0
    assert torch.equal(cbit, first[0]) and torch.equal(uoff, first[1]) and torch.equal(state, first[2])
    st = eng.results_to_host(streams, pkg.CHECKPOINT_STREAM_DTYPE)
    assert (st == first[4]).all() and sum(1 for s in st if s["status"] == pkg.CPS_OK) == 15 * 7


# ---- range reads ------------------------------------------------------------------------------------------------------------------
class Indexed:
    """one stream of the batch with index, states and windows as the device wrote them"""

    def __init__(self, batch, halves, name, span):
        sub, fmt = halves[0] if name in halves[0][0].names else halves[1]
        k = sub.names.index(name)
        m = sub.model[span][k]
        cbit, uoff, state, windows, st = sub.index(fmt, span, m["count"], windows=True, dst=sub.dst)
        assert st[k]["status"] == pkg.CPS_OK and st[k]["count"] == m["count"]
        self.eng, self.m, self.plain, self.length, self.stream = batch.eng, m, sub.plain[k], len(sub.stream[k]), sub.stream[k]
        self.src = sub.src[sub.sat[k]:sub.sat[k] + self.length].clone()
        self.cbit, self.uoff, self.state, self.windows = cbit[k].clone(), uoff[k].clone(), state[k].clone(), windows[k].clone()

    def read(self, ranges, dst=None, src=None, state=None):
        import torch
        r = torch.tensor(np.array(ranges, np.uint64).reshape(-1, 2).view(np.int64), device=self.eng.dev)
        rc, offs, st, out_len, decoded, dst = self.eng.checkpoint_read_ranges_fine(self.src if src is None else src, self.length, self.cbit, self.uoff,
                                                                                   self.state if state is None else state, self.windows, r, dst)
        torch.cuda.synchronize(self.eng.dev)
        return rc, offs.cpu().numpy(), st.cpu().numpy(), out_len, decoded, dst

    def segments_of(self, ranges):
        u, L, out = self.m["uoff"], self.m["count"], set()
        for b, e in ranges:
            if b < e <= u[L]:
                out |= set(range(bisect.bisect_right(u[:L], b) - 1, bisect.bisect_right(u[:L], e - 1)))
        return out


def ranges_for(m, rnd):
    """64 ranges: random ones, ranges that straddle segments, the whole stream, empty ones, one out of bounds"""
    u, L, n = m["uoff"], m["count"], m["out_len"]
    mid = L // 2
    r = [(u[mid] + 5, u[mid] + 105), (u[mid + 1] - 3, u[mid + 1] + 3), (0, n), (n - 1, n), (0, 1), (7, 7), (n, n), (0, 0), (n - 5, n + 1),
         (u[1] + 1, u[min(6, L)] - 1), (u[mid] - 1, u[min(mid + 4, L)])]
    ks = list(range(1, L))
    rnd.shuffle(ks)
    for k in ks[:10]:
        r += [(u[k] - 1, u[k]), (u[k], u[k] + 1), (u[k] - 1, u[k] + 1)]
    while len(r) < 64:
        b = rnd.randrange(0, n)
        r.append((b, min(n, b + rnd.choice([1, 100, 20000]))))
    return r[:64]


def check_read(ix, ranges, rc, offs, st, out_len, decoded, dst, damaged=()):
    n = ix.m["out_len"]
    assert rc == 0
    exp_len = [e - b if b <= e <= n else 0 for b, e in ranges]
    assert offs.tolist() == [sum(exp_len[:k]) for k in range(len(ranges) + 1)] and out_len == sum(exp_len)
    got = dst.cpu().numpy()
    for k, (b, e) in enumerate(ranges):
        bad = not (b <= e <= n)
        hit = not bad and bool(ix.segments_of([(b, e)]) & set(damaged))
        assert st[k] == (pkg.RANGE_OUT_OF_BOUNDS if bad else pkg.RANGE_DAMAGED if hit else pkg.RANGE_OK), (k, b, e, st[k])
        piece = got[offs[k]:offs[k + 1]].tobytes()
        assert piece == (bytes(exp_len[k]) if hit else ix.plain[b:e] if not bad else b""), (k, b, e)
    assert decoded == len(ix.segments_of(ranges))


READS = [("fixed_one_block", 1000), ("alice6_gzip_fields", 4096), ("stored", 4096), ("rle_zeros", 1000), ("mem1", 258), ("mem9", 65536),
         ("engine", 4096), ("empty_final_block", 4096), ("alice1", 258)]


@pytest.fixture(scope="module")
def indexed(batch, halves):
    return {key: Indexed(batch, halves, *key) for key in READS}


@pytest.mark.parametrize("name,span", READS)
def test_ranges_equal_the_plain_slices(indexed, monkeypatch, name, span):
    ix = indexed[(name, span)]
    m = ix.m
    ranges = ranges_for(m, random.Random(len(name) + span))
    want = ix.read(ranges)
    check_read(ix, ranges, *want)
    # one byte from every segment: each is decoded, once
    every = [(u, u + 1) for u in m["uoff"][:m["count"]] if u < m["out_len"]]
    res = ix.read(every)
    check_read(ix, every, *res)
    assert res[4] == len(every) >= m["count"] - 1
    # one byte from the middle: one segment
    one = [(m["out_len"] // 2, m["out_len"] // 2 + 1)]
    res = ix.read(one)
    check_read(ix, one, *res)
    assert res[4] == 1
    # several chunks of segments: the same
    monkeypatch.setenv("NXZ_BGZF_CHUNK", "7")
    res = ix.read(ranges)
    check_read(ix, ranges, *res)
    assert res[5].cpu().numpy()[:res[3]].tobytes() == want[5].cpu().numpy()[:want[3]].tobytes()


@pytest.mark.parametrize("knob,value", [("NXZ_INFLATE_LANES_MIN", "1"), ("NXZ_INFLATE_WG", "0")])
def test_no_route_that_ignores_the_suspend_flag(indexed, monkeypatch, knob, value):
    """the segments' jobs rely on NXZ_JOB_SUSPEND_WHEN_FULL: with the knobs that name another decode route the reads are the same"""
    monkeypatch.setenv(knob, value)
    for key in (("fixed_one_block", 1000), ("alice1", 258)):
        ix = indexed[key]
        ranges = ranges_for(ix.m, random.Random(11))
        check_read(ix, ranges, *ix.read(ranges))


def test_a_flipped_source_byte_damages_what_depends_on_it_and_no_more(indexed):
    """no checksum is compared: the byte is one whose damage a decoder must notice -- LEN of a stored block; HLIT of a table, which
    damages the segment the header lies in and every segment that resumes inside that block (its state names that table)"""
    import torch
    # the stored stream: the second block's LEN, inside some segment
    ix = indexed[("stored", 4096)]
    m = ix.m
    hdr = F.walk_cached(ix.stream, F.FMT_ZLIB)[1][1][0]
    byte = ((hdr + 3 + 7) >> 3)
    k = bisect.bisect_right(m["cbit"][:m["count"]], 8 * byte) - 1
    assert m["cbit"][k] < hdr and 8 * byte + 32 <= m["cbit"][k + 1]
    host = ix.src.cpu().numpy().copy()
    host[byte] ^= 0x10
    ranges = ranges_for(m, random.Random(5)) + [(m["uoff"][k], m["uoff"][k] + 1), (m["uoff"][k + 1] - 1, m["uoff"][k + 1] + 1)]
    res = ix.read(ranges, src=torch.from_numpy(host).to(ix.eng.dev))
    check_read(ix, ranges, *res, damaged=(k,))
    assert (res[2] == pkg.RANGE_DAMAGED).sum() >= 2 and (res[2] == pkg.RANGE_OK).sum() >= 30
    # a dynamic table in the middle of the many-blocks stream
    ix = indexed[("mem1", 258)]
    m = ix.m
    headers = F.walk_cached(ix.stream, F.FMT_GZIP)[1]
    host = ix.src.cpu().numpy().copy()
    bits = lambda p, n: sum(((int(host[(p + i) >> 3]) >> ((p + i) & 7)) & 1) << i for i in range(n))
    hdr = next(h for h, _ in headers[len(headers) // 2:] if bits(h + 1, 2) == 2)
    for p in range(hdr + 3, hdr + 8):                                      # HLIT becomes 31: 288 codes, two more than there are
        host[p >> 3] |= 1 << (p & 7)
    L = m["count"]
    damaged = {bisect.bisect_right(m["cbit"][:L], hdr) - 1} | {j for j in range(L) if m["state"][j][0] == hdr + 3}
    assert 2 <= len(damaged) <= 8
    lo, hi = min(damaged), max(damaged)
    ranges = ranges_for(m, random.Random(6)) + [(m["uoff"][j], m["uoff"][j] + 1) for j in range(max(lo - 2, 0), min(hi + 3, L))]
    res = ix.read(ranges, src=torch.from_numpy(host).to(ix.eng.dev))
    check_read(ix, ranges, *res, damaged=damaged)
    assert (res[2] == pkg.RANGE_DAMAGED).sum() >= len(damaged) and (res[2] == pkg.RANGE_OK).sum() >= 30


def test_broken_state_entries_are_refused(indexed):
    import torch
    seen = set()
    for key in (("alice6_gzip_fields", 4096), ("stored", 4096), ("fixed_one_block", 1000)):
        ix = indexed[key]
        ranges = [(0, 1000), (50000, 60000)]
        for what, b in F.broken_states(ix.m):
            seen.add(what)
            keep = ix.cbit
            ix.cbit = torch.tensor(b["cbit"], dtype=torch.int64, device=ix.eng.dev)
            state = torch.from_numpy(np.array(b["state"], dtype=STATE).view(np.uint8).copy()).to(ix.eng.dev)
            dst = torch.full((11000,), PATTERN, dtype=torch.uint8, device=ix.eng.dev)
            try:
                rc, offs, st, out_len, decoded, _ = ix.read(ranges, dst=dst, state=state)
            finally:
                ix.cbit = keep
            assert rc == -errno.EILSEQ and out_len == 0 and decoded == 0 and bool((dst == PATTERN).all()), (key, what)
        rc, _, _, _, decoded, _ = ix.read(ranges)
        assert rc == 0 and decoded == len(ix.segments_of(ranges))
    assert len(seen) >= 19


def test_a_coarse_index_with_zero_states_reads_what_the_coarse_call_reads(eng, batch, halves):
    import torch
    for name in ("mem1", "alice6_raw"):
        sub, fmt = halves[0] if name in halves[0][0].names else halves[1]
        k = sub.names.index(name)
        rc, cbit, uoff, windows, streams = eng.checkpoint_index(fmt, sub.jobs(sub.dst), sub.n, 16384, 32, windows=True)
        cnt = int(eng.results_to_host(streams, pkg.CHECKPOINT_STREAM_DTYPE)[k]["count"])
        assert rc == 0 and 1 <= cnt <= 32
        src = sub.src[sub.sat[k]:sub.sat[k] + len(sub.stream[k])].clone()
        cb, uo, wi = cbit[k, :cnt + 1].contiguous(), uoff[k, :cnt + 1].contiguous(), windows[k, :cnt].contiguous()
        n = len(sub.plain[k])
        rnd = random.Random(9)
        ranges = [(0, n), (n // 2, n // 2 + 1), (5, 5)] + [(b, min(n, b + 30000)) for b in (rnd.randrange(n) for _ in range(20))]
        r = torch.tensor(np.array(ranges, np.int64), device=eng.dev)
        a = eng.checkpoint_read_ranges(src, len(sub.stream[k]), cb, uo, wi, r)
        zero = torch.zeros((cnt + 1) * STATE.itemsize, dtype=torch.uint8, device=eng.dev)
        b = eng.checkpoint_read_ranges_fine(src, len(sub.stream[k]), cb, uo, zero, wi, r)
        torch.cuda.synchronize(eng.dev)
        assert a[0] == b[0] == 0 and a[3] == b[3] and a[4] == b[4] and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
        assert torch.equal(a[5][:a[3]], b[5][:b[3]]) and a[5][:n].cpu().numpy().tobytes() == sub.plain[k]


def test_a_chain_of_suspended_jobs_stops_at_the_checkpoints(eng, batch):
    """nxz_batch_decompress with NXZ_JOB_SUSPEND_WHEN_FULL and dst_cap = span, job after job from where the last one suspended:
    the places are the index's -- bit (spbc, subc), sfbt, rem and dhtlen"""
    import torch
    span = 4096
    for name in ("alice6_raw", "stored"):
        i = batch.names.index(name)
        m, stream, plain = batch.model[span][i], batch.stream[i], batch.plain[i]
        hdr = m["hdr_len"]
        dht = torch.zeros(pkg.engine.DHT_DTYPE.itemsize, dtype=torch.uint8, device=eng.dev)
        out = torch.zeros(span + 16, dtype=torch.uint8, device=eng.dev)
        bit, resume, u = 8 * hdr, 0, 0
        for k in range(1, m["count"] + 1):
            b = bit >> 3
            w = min(u, W)
            buf = np.zeros(((w + 15) & ~15) + len(stream) - b + 16, np.uint8)
            pad = (-w) & 15
            buf[pad:pad + w] = np.frombuffer(plain[u - w:u], np.uint8)
            buf[pad + w:pad + w + len(stream) - b] = np.frombuffer(stream[b:], np.uint8)
            src = torch.from_numpy(buf).to(eng.dev)
            j = np.zeros(1, pkg.JOB_DTYPE)
            j[0]["src"], j[0]["src_len"], j[0]["hist_len"] = src.data_ptr() + pad, w + len(stream) - b, w
            j[0]["dst"], j[0]["dst_cap"], j[0]["in_adler"] = out.data_ptr(), span, 1
            j[0]["resume"], j[0]["reserved"] = resume | ((8 - (bit & 7)) & 7) << 20, pkg.JOB_SUSPEND_WHEN_FULL
            r = eng.results_to_host(eng.decompress(eng.to_device(j), 1, dht_io=dht))[0]
            last = k == m["count"]
            assert r["cc"] == 3 or (last and r["cc"] == 0), (name, k, r)     # (the last: 3 too when a trailer follows the final block)
            assert r["tpbc"] == m["uoff"][k] - m["uoff"][k - 1] and out[:int(r["tpbc"])].cpu().numpy().tobytes() == plain[u:u + int(r["tpbc"])], (name, k)
            u += int(r["tpbc"])
            if last:
                break
            bit = 8 * (b + int(r["spbc"]) - w) - int(r["subc"])
            tbit, res, dhtlen = m["state"][k]
            sfbt = int(r["sfbt"]) & 15
            assert bit == m["cbit"][k] and sfbt == (res >> 16) & 15 and int(r["tebc"]) == res & 0xffff, (name, k, bit, m["cbit"][k], r)
            assert (int(r["sfbt"]) >> 16) & 0xfff == dhtlen, (name, k, r)
            if dhtlen:
                t = eng.results_to_host(dht, pkg.engine.DHT_DTYPE)[0]
                assert t["dhtlen"] == dhtlen and t["dht"].tobytes()[:(dhtlen + 7) // 8] == F.table_bits(stream, tbit, dhtlen), (name, k)
            resume = int(r["tebc"]) | sfbt << 16
