"""GPU tests of the checkpoint calls (include/nxz_engine.h: nxz_batch_checkpoint_index, nxz_checkpoint_read_ranges; kernels in
power-gzip_amd/csrc/nxz_checkpoint.hip): ONE batch of raw, zlib and gzip streams of 150-250 KiB of plain bytes each -- zlib's at
memLevel 1 (hundreds of blocks, most of them starting inside a byte) and 8, stored and fixed-code streams, one the engine wrote
itself, an empty one, one cut short, one with a damaged table -- indexed with spans of 16 KiB and 1 against the model
(tests/checkpoint_model.py: block headers from system zlib's inflate(Z_BLOCK)), with and without windows; then ranges of three of
them read through index and windows alone, against slices of the plain bytes."""
import bisect
import errno
import importlib
import os
import random
import struct
import zlib

import numpy as np
import pytest

import checkpoint_model as M
from datagen import ALICE_LIKE, make_block

pytestmark = pytest.mark.gpu
pkg = importlib.import_module("power-gzip_amd")
KNOBS = ("NXZ_INFLATE_LANES_MIN", "NXZ_INFLATE_CUT", "NXZ_INFLATE_WG", "NXZ_INFLATE_WG_MAX", "NXZ_WG_PMIN", "NXZ_INFLATE_ORDER",
         "NXZ_BGZF_CHUNK", "NXZ_STREAMS_CHUNK")
W = M.WINDOW
PATTERN = 0xA5
SPANS = (16384, 1)


@pytest.fixture(scope="module")
def eng():
    saved = {k: os.environ.pop(k, None) for k in KNOBS}
    e = pkg.Engine(0)
    yield e
    e.close()
    for k, v in saved.items():
        if v is not None:
            os.environ[k] = v


def gzip_with_fields(data, level, mem_level):
    """a gzip member with FEXTRA and FNAME in front of the deflate data"""
    extra = b"XY\x05\x00hello"
    head = b"\x1f\x8b\x08" + bytes([4 | 8]) + bytes(4) + b"\x00\x03" + struct.pack("<H", len(extra)) + extra + b"pages.log\x00"
    return head + M.deflate(data, M.FMT_RAW, level, mem_level) + struct.pack("<II", zlib.crc32(data), len(data) & 0xffffffff)


def engine_stream(eng, data):
    """data as nxz_batch_deflate_streams writes it: a zlib stream of 64 KiB blocks"""
    import torch
    buf = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).to(eng.dev)
    out, offsets, results = eng.deflate_streams(pkg.FC_COMPRESS_DHTGEN, pkg.FMT_ZLIB, [buf])
    r = eng.results_to_host(results, pkg.engine.STREAM_RESULT_DTYPE)[0]
    assert r["cc"] == 0
    return out[:int(r["out_len"])].cpu().numpy().tobytes()


class Batch:
    """the streams on the device, 16-byte aligned, and per stream a target slot for its decoded output"""

    def __init__(self, eng):
        import torch
        alice = ALICE_LIKE(200000)
        s = []                                                            # (name, fmt, stream, plain)

        def add(name, fmt, stream, plain):
            s.append((name, fmt, stream, plain))
        lz, al4, al2 = make_block("lz", 163841, seed=3), make_block("alice", 250000, seed=4), make_block("alice", 153601, seed=5)
        add("raw-1", M.FMT_RAW, M.deflate(alice, M.FMT_RAW, 1, 1), alice)
        add("raw-9", M.FMT_RAW, M.deflate(lz, M.FMT_RAW, 9, 1), lz)
        add("zlib-6", M.FMT_ZLIB, M.deflate(alice, M.FMT_ZLIB, 6, 1), alice)
        add("zlib-1", M.FMT_ZLIB, M.deflate(al4, M.FMT_ZLIB, 1, 1), al4)
        add("gzip-6-fields", M.FMT_GZIP, gzip_with_fields(alice, 6, 1), alice)
        add("gzip-9", M.FMT_GZIP, M.deflate(al2, M.FMT_GZIP, 9, 1), al2)
        add("zlib-6-mem8", M.FMT_ZLIB, M.deflate(alice, M.FMT_ZLIB, 6, 8), alice)
        add("zlib-0", M.FMT_ZLIB, M.deflate(al2, M.FMT_ZLIB, 0, 1), al2)
        add("zlib-fixed", M.FMT_ZLIB, M.deflate(alice, M.FMT_ZLIB, 6, 1, zlib.Z_FIXED), alice)
        add("engine", M.FMT_ZLIB, engine_stream(eng, alice), alice)
        add("empty", M.FMT_GZIP, M.deflate(b"", M.FMT_GZIP), b"")
        z = M.deflate(alice, M.FMT_ZLIB, 6, 1)
        add("cut", M.FMT_ZLIB, z[:len(z) * 3 // 5], None)
        bad = bytearray(z)
        assert (bad[2] >> 1) & 3 == 2                                     # the first block brings a table ...
        bad[2] |= 0xf8                                                    # ... of 288 literal / length codes: two more than there are
        add("table", M.FMT_ZLIB, bytes(bad), None)
        self.names = [x[0] for x in s]
        self.fmt = [x[1] for x in s]
        self.stream = [x[2] for x in s]
        self.plain = [x[3] for x in s]
        self.n = n = len(s)
        self.eng = eng
        self.model = {span: [M.index(st, f, span) for st, f in zip(self.stream, self.fmt)] for span in SPANS}
        for span in SPANS:
            for i, m in enumerate(self.model[span]):
                assert (m is None) == (self.plain[i] is None) and (m is None or m["plain"] == self.plain[i]), self.names[i]
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
        self.dst = torch.from_numpy(hd).to(eng.dev)                       # the decoded outputs (the plain bytes), canary between them

    def jobs(self, dst=None, cap=None, **fields):
        j = np.zeros(self.n, pkg.JOB_DTYPE)
        for i in range(self.n):
            j[i]["src"] = self.src.data_ptr() + self.sat[i]
            j[i]["src_len"] = len(self.stream[i])
            j[i]["dst"] = 0 if dst is None else dst.data_ptr() + self.dat[i]
            j[i]["dst_cap"] = (self.cap if cap is None else cap)[i]
            j[i]["in_adler"] = 1
        for k, v in fields.items():
            j[k] = v
        return self.eng.to_device(j)

    def index(self, fmt, span, cp_cap, windows=False, dst=None, cap=None, **fields):
        import torch
        eng = self.eng
        if windows:
            windows = torch.full((self.n, cp_cap, W), PATTERN, dtype=torch.uint8, device=eng.dev)
        cbit = torch.full((self.n, cp_cap + 1), -1, dtype=torch.int64, device=eng.dev)
        uoff = torch.full((self.n, cp_cap + 1), -1, dtype=torch.int64, device=eng.dev)
        rc, cbit, uoff, windows, streams = eng.checkpoint_index(fmt, self.jobs(dst, cap, **fields), self.n, span, cp_cap, windows, cbit, uoff)
        assert rc == 0
        st = eng.results_to_host(streams, pkg.CHECKPOINT_STREAM_DTYPE)[:self.n]
        return cbit, uoff, windows, st


@pytest.fixture(scope="module")
def batch(eng):
    return Batch(eng)


def check_positions(batch, span, cp_cap, cbit, uoff, st, no_output=()):
    """streams[], cbit and uoff against the model; entries behind what a stream stores still hold the fill (-1)"""
    cb, uo = cbit.cpu().numpy(), uoff.cpu().numpy()
    for i, m in enumerate(batch.model[span]):
        name, s = batch.names[i], st[i]
        if m is None:
            assert s["status"] == pkg.CPS_STREAM_FAILED and s["count"] == 0 and s["cc"] != 0 and s["out_len"] == 0, (name, s)
            assert (s["frame_status"], s["cc"] == 3) == ((pkg.FRAME_TRUNCATED, True) if name == "cut" else (pkg.FRAME_DEFLATE, False)), (name, s)
            continue
        exp = pkg.CPS_MORE if m["count"] > cp_cap else pkg.CPS_NO_OUTPUT if i in no_output else pkg.CPS_OK
        assert (s["status"], s["count"], s["out_len"], s["cc"], s["frame_status"]) == (exp, m["count"], m["out_len"], 0, pkg.FRAME_OK), (name, s, m["count"])
        assert s["format"] == batch.fmt[i] and s["hdr_len"] == m["cbit"][0] // 8, (name, s)
        k = min(m["count"], cp_cap) + (0 if exp == pkg.CPS_MORE else 1)     # (with the sentinel, unless checkpoints were only counted)
        assert cb[i, :k].tolist() == m["cbit"][:k] and uo[i, :k].tolist() == m["uoff"][:k], name
        assert (cb[i, k:] == -1).all() and (uo[i, k:] == -1).all(), name


def check_windows(batch, span, cp_cap, windows, written):
    """the window of every stored checkpoint of the streams in `written` is the plain slice in front of it; every other byte of the
    slots still holds the fill"""
    w = windows.cpu().numpy()
    for i, m in enumerate(batch.model[span]):
        stored = min(m["count"], cp_cap) if (m is not None and i in written) else 0
        for k in range(stored):
            u = m["uoff"][k]
            n = min(u, W)
            assert w[i, k, :n].tobytes() == batch.plain[i][u - n:u], (batch.names[i], k)
            assert (w[i, k, n:] == PATTERN).all(), (batch.names[i], k)
        assert (w[i, stored:] == PATTERN).all(), batch.names[i]


@pytest.fixture(scope="module")
def counts(batch):
    return {span: max(m["count"] for m in batch.model[span] if m is not None) for span in SPANS}


class Sub:
    """the raw streams, or the framed ones, of the batch as a batch of its own (raw streams have no header to tell them by)"""

    def __init__(self, batch, pick):
        self.__dict__.update(batch.__dict__)
        self.ids = pick
        for f in ("names", "fmt", "stream", "plain", "sat", "dat", "cap"):
            setattr(self, f, [getattr(batch, f)[i] for i in pick])
        self.model = {span: [batch.model[span][i] for i in pick] for span in SPANS}
        self.n = len(pick)
    jobs = Batch.jobs
    index = Batch.index


@pytest.fixture(scope="module")
def halves(batch):
    raw = [i for i in range(batch.n) if batch.fmt[i] == M.FMT_RAW]
    framed = [i for i in range(batch.n) if batch.fmt[i] != M.FMT_RAW]
    assert len(raw) == 2 and len(framed) == 11
    return ((Sub(batch, raw), pkg.engine.FMT_RAW), (Sub(batch, framed), pkg.FMT_AUTO))


def test_the_batch_is_what_the_issue_asks_for(batch, counts):
    assert batch.n == 13 and all(p is None or p == b"" or 150000 <= len(p) <= 256000 for p in batch.plain)
    m16 = {n: m for n, m in zip(batch.names, batch.model[16384])}
    m1 = {n: m for n, m in zip(batch.names, batch.model[1])}
    assert 8 <= m16["zlib-6"]["count"] <= 16 and m1["zlib-6"]["count"] > 200 and m1["raw-1"]["count"] > 300
    assert sum(1 for c in m1["zlib-6"]["cbit"] if c & 7) > 150           # most headers stand inside a byte
    assert m1["zlib-6-mem8"]["count"] <= 4 and m1["engine"]["count"] >= 3
    assert m1["empty"]["count"] == 1 and m1["empty"]["uoff"] == [0, 0]
    assert m1["gzip-6-fields"]["cbit"][0] == 8 * (10 + 2 + 9 + 10)


@pytest.mark.parametrize("span", SPANS)
def test_positions_and_windows_equal_the_model(halves, counts, span):
    cp_cap = counts[span] + 1
    for sub, fmt in halves:
        cbit, uoff, windows, st = sub.index(fmt, span, cp_cap, windows=True, dst=sub.dst)
        check_positions(sub, span, cp_cap, cbit, uoff, st)
        check_windows(sub, span, cp_cap, windows, set(range(sub.n)))


def test_explicit_formats_equal_auto(halves):
    sub, _ = halves[1]
    for fmt, want in ((pkg.FMT_ZLIB, M.FMT_ZLIB), (pkg.FMT_GZIP, M.FMT_GZIP)):
        _, _, _, st = sub.index(fmt, 16384, 16)
        for i in range(sub.n):
            ok = sub.model[16384][i] is not None and sub.fmt[i] == want
            assert (st[i]["status"] == pkg.CPS_OK) == ok, (fmt, sub.names[i], st[i])
            assert ok or (st[i]["status"] == pkg.CPS_STREAM_FAILED and st[i]["count"] == 0), (fmt, sub.names[i], st[i])


def test_a_small_cap_counts_on(halves, batch):
    span = 16384
    for sub, fmt in halves:
        cp_cap = sub.model[span][0]["count"] - 1                          # one below the first stream's count
        assert cp_cap >= 2
        cbit, uoff, windows, st = sub.index(fmt, span, cp_cap, windows=True, dst=sub.dst)
        assert st[0]["status"] == pkg.CPS_MORE and st[0]["count"] == cp_cap + 1
        assert any(s["status"] == pkg.CPS_OK for s in st)
        check_positions(sub, span, cp_cap, cbit, uoff, st)
        check_windows(sub, span, cp_cap, windows, set(range(sub.n)))


def test_without_windows_dst_is_never_touched(halves, batch):
    import torch
    for sub, fmt in halves:
        scratch = torch.full_like(batch.dst, PATTERN)
        for dst, cap in ((scratch, None), (None, None), (scratch, [0] * sub.n)):
            cbit, uoff, windows, st = sub.index(fmt, 16384, 16, windows=False, dst=dst, cap=cap)
            assert windows is None
            check_positions(sub, 16384, 16, cbit, uoff, st)
        assert bool((scratch == PATTERN).all())


def test_a_short_target_keeps_the_positions(halves, batch):
    for sub, fmt in halves:
        cap = list(sub.cap)
        short = [i for i in (0, 1) if sub.plain[i]]
        for i in short:
            cap[i] -= 1
        import torch
        cbit, uoff, windows, st = sub.index(fmt, 16384, 16, windows=True, dst=sub.dst, cap=cap)
        check_positions(sub, 16384, 16, cbit, uoff, st, no_output=set(short))
        check_windows(sub, 16384, 16, windows, set(range(sub.n)) - set(short))
        # ... and a NULL target
        cbit, uoff, windows, st = sub.index(fmt, 16384, 16, windows=True, dst=None)
        check_positions(sub, 16384, 16, cbit, uoff, st, no_output=set(range(sub.n)))
        check_windows(sub, 16384, 16, windows, set())
        assert torch.equal(batch.dst.cpu(), torch.from_numpy(batch.dst_host))


def test_refusals(eng, halves):
    sub, fmt = halves[1]
    for field, value in (("hist_len", 16), ("resume", 3 << 20)):
        v = np.zeros(sub.n, np.uint32)
        v[1] = value
        cbit, uoff, _, st = sub.index(fmt, 16384, 16, **{field: v})
        assert st[1]["status"] == pkg.CPS_INVALID and st[1]["count"] == 0 and st[1]["out_len"] == 0
        assert (cbit[1] == -1).all() and st[0]["status"] == pkg.CPS_OK and st[2]["status"] == pkg.CPS_OK
    jobs = sub.jobs()
    for args in ((fmt, jobs, sub.n, 0, 16), (fmt, jobs, sub.n, 16384, 0), (7, jobs, sub.n, 16384, 16), (-1, jobs, sub.n, 16384, 16)):
        assert eng.checkpoint_index(*args)[0] == -errno.EINVAL
    assert eng.checkpoint_index(fmt, None, 0, 16384, 16)[0] == 0
    assert eng.L.nxz_batch_checkpoint_index(eng.ctx, fmt, None, 3, 16384, 16, None, None, None, None, eng.stream_handle()) == -errno.EINVAL


# ---- range reads ------------------------------------------------------------------------------------------------------------------
class Indexed:
    """one stream of the batch with index and windows as the device wrote them (the decoded output is not used from here on)"""

    def __init__(self, batch, name, span):
        i = batch.names.index(name)
        raw = batch.fmt[i] == M.FMT_RAW
        pick = [k for k in range(batch.n) if (batch.fmt[k] == M.FMT_RAW) == raw]
        sub = Sub(batch, pick)
        m = batch.model[span][i]
        cbit, uoff, windows, st = sub.index(pkg.engine.FMT_RAW if raw else pkg.FMT_AUTO, span, m["count"], windows=True, dst=sub.dst)
        k = pick.index(i)
        assert st[k]["status"] == pkg.CPS_OK and st[k]["count"] == m["count"]
        self.eng, self.m, self.plain, self.length = batch.eng, m, batch.plain[i], len(batch.stream[i])
        self.src = batch.src[batch.sat[i]:batch.sat[i] + self.length].clone()
        self.cbit, self.uoff, self.windows = cbit[k].clone(), uoff[k].clone(), windows[k].clone()

    def read(self, ranges, dst=None, src=None, cbit=None, uoff=None):
        import torch
        r = torch.tensor(np.array(ranges, np.uint64).reshape(-1, 2).view(np.int64), device=self.eng.dev)
        rc, offs, st, out_len, decoded, dst = self.eng.checkpoint_read_ranges(self.src if src is None else src, self.length,
                                                                              self.cbit if cbit is None else cbit,
                                                                              self.uoff if uoff is None else uoff, self.windows, r, dst)
        torch.cuda.synchronize(self.eng.dev)
        return rc, offs.cpu().numpy(), st.cpu().numpy(), out_len, decoded, dst

    def segments_of(self, ranges):
        """the distinct segments the ranges that are in bounds and not empty touch"""
        u, L, out = self.m["uoff"], self.m["count"], set()
        for b, e in ranges:
            if b < e <= u[L]:
                out |= set(range(bisect.bisect_right(u[:L], b) - 1, bisect.bisect_right(u[:L], e - 1)))
        return out


def ranges_for(m, rnd):
    """64 ranges: inside one segment, across two and five, the whole stream, a byte on each side of every checkpoint (as many as
    fit), empty ones, out of bounds, duplicates and overlaps"""
    u, L, n = m["uoff"], m["count"], m["out_len"]
    mid = L // 2
    r = [(u[mid] + 5, u[mid] + 105), (u[mid + 1] - 3, u[mid + 1] + 3), (0, n), (n - 1, n), (0, 1),
         (7, 7), (n, n), (0, 0), (9, 8), (n - 5, n + 1), (n + 1, n + 2), ((1 << 63) + 5, 7)]
    if L >= 6:
        r += [(u[1] + 1, u[6] - 1), (u[mid] - 1, u[min(mid + 4, L)] + 1 if mid + 4 < L else n)]
    r += [r[0], r[1], (u[mid] + 50, u[mid] + 80), (u[mid] + 60, u[mid + 1] + 10)]                 # duplicates and overlaps
    ks = list(range(1, L))
    rnd.shuffle(ks)
    for k in ks:
        if len(r) + 3 > 64:
            break
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


@pytest.fixture(scope="module")
def indexed(batch):
    return {(name, span): Indexed(batch, name, span) for name, span in (("raw-1", 16384), ("gzip-6-fields", 16384), ("zlib-6", 1), ("engine", 1))}


@pytest.mark.parametrize("name,span,chunk", [("raw-1", 16384, None), ("gzip-6-fields", 16384, "3"), ("zlib-6", 1, "50"), ("engine", 1, None)])
def test_ranges_equal_the_plain_slices(indexed, monkeypatch, name, span, chunk):
    ix = indexed[(name, span)]
    if chunk:
        monkeypatch.setenv("NXZ_BGZF_CHUNK", chunk)                       # several chunks of segments
    ranges = ranges_for(ix.m, random.Random(len(name) + span))
    assert len(ranges) == 64 and (ix.m["count"] < 6 or len(ix.segments_of(ranges)) == ix.m["count"])
    check_read(ix, ranges, *ix.read(ranges))
    # a few ranges of one segment: that segment alone is decoded
    u = ix.m["uoff"]
    few = [(u[1] + 1, u[1] + 2), (u[1] + 1, u[2]), (u[1], u[1] + 9)]
    res = ix.read(few)
    check_read(ix, few, *res)
    assert res[4] == 1


def test_a_small_target_is_e2big(indexed):
    import torch
    ix = indexed[("raw-1", 16384)]
    ranges = [(10, 5010), (100000, 100100)]
    dst = torch.full((5099,), PATTERN, dtype=torch.uint8, device=ix.eng.dev)
    rc, offs, st, out_len, decoded, _ = ix.read(ranges, dst=dst)
    assert rc == -errno.E2BIG and out_len == 5100 and decoded == 0 and offs.tolist() == [0, 5000, 5100] and st.tolist() == [0, 0]
    assert bool((dst == PATTERN).all())


def test_a_flipped_source_byte_damages_its_segment_alone(indexed):
    ix = indexed[("zlib-6", 1)]
    m = ix.m
    k = m["count"] // 2
    c = m["cbit"][k]
    src = ix.src.clone()
    host = src.cpu().numpy()
    bits = lambda p, n: sum(((host[(p + i) >> 3] >> ((p + i) & 7)) & 1) << i for i in range(n))
    assert bits(c + 1, 2) == 2                                            # segment k begins with a table ...
    byte = (c + 3) >> 3                                                   # ... whose HLIT field (bits c + 3 .. c + 7) becomes 31
    for p in range(c + 3, c + 8):
        host[p >> 3] |= 1 << (p & 7)
    assert m["cbit"][k] >> 3 <= byte < (m["cbit"][k + 1] + 7) >> 3 and bits(c + 3, 5) == 31
    src.copy_(ix.eng.torch.from_numpy(host))
    ranges = ranges_for(m, random.Random(77)) + [(m["uoff"][k], m["uoff"][k] + 1), (m["uoff"][k + 1] - 1, m["uoff"][k + 1]),
                                                  (m["uoff"][k] - 1, m["uoff"][k]), (m["uoff"][k + 1], m["uoff"][k + 1] + 1)]
    res = ix.read(ranges, src=src)
    check_read(ix, ranges, *res, damaged=(k,))
    assert (res[2] == pkg.RANGE_DAMAGED).sum() >= 3 and (res[2] == pkg.RANGE_OK).sum() >= 40


def test_a_foreign_index_is_refused(indexed):
    import torch
    ix = indexed[("gzip-6-fields", 16384)]
    L = ix.m["count"]
    ranges = [(0, 1000), (50000, 60000)]

    def refused(cbit=None, uoff=None, length=None):
        dst = torch.full((11000,), PATTERN, dtype=torch.uint8, device=ix.eng.dev)
        keep = ix.length
        if length is not None:
            ix.length = length
        try:
            rc, offs, st, out_len, decoded, _ = ix.read(ranges, dst=dst, cbit=cbit, uoff=uoff)
        finally:
            ix.length = keep
        assert rc == -errno.EILSEQ and out_len == 0 and decoded == 0 and bool((dst == PATTERN).all())
    for which in ("cbit", "uoff"):
        t = getattr(ix, which).clone()
        t[[2, 3]] = t[[3, 2]]                                             # swapped
        refused(**{which: t})
        t = getattr(ix, which).clone()
        t[L - 1] = t[1]                                                   # decreasing
        refused(**{which: t})
    t = ix.uoff.clone()
    t[0] = 1
    refused(uoff=t)
    t = ix.cbit.clone()
    t[L] = 8 * ix.length + 1                                              # the sentinel beyond the source
    refused(cbit=t)
    refused(length=(ix.m["cbit"][L] + 7) // 8 - 1)                        # ... a source shorter than the index says
    rc, offs, st, out_len, decoded, dst = ix.read(ranges)                 # (and the index itself is fine)
    assert rc == 0 and decoded == len(ix.segments_of(ranges))


def test_the_recipe_decode_index_drop_read(eng, batch):
    """decode once with nxz_batch_decompress_framed, index with windows from that output, drop the output, read ranges"""
    import torch
    i = batch.names.index("gzip-9")
    plain, stream = batch.plain[i], batch.stream[i]
    src = batch.src[batch.sat[i]:batch.sat[i] + len(stream)]
    out = torch.zeros(len(plain) + 16, dtype=torch.uint8, device=eng.dev)
    j = np.zeros(1, pkg.JOB_DTYPE)
    j[0]["src"], j[0]["src_len"], j[0]["dst"], j[0]["dst_cap"], j[0]["in_adler"] = src.data_ptr(), len(stream), out.data_ptr(), len(plain), 1
    jobs = eng.to_device(j)
    results, frames = eng.decompress_framed(pkg.FMT_AUTO, jobs, 1)
    cp_cap = 32
    rc, cbit, uoff, windows, streams = eng.checkpoint_index(pkg.FMT_AUTO, jobs, 1, 16384, cp_cap, windows=True)
    assert rc == 0 and eng.frames_to_host(frames)[0]["status"] == pkg.FRAME_OK
    s = eng.results_to_host(streams, pkg.CHECKPOINT_STREAM_DTYPE)[0]
    m = batch.model[16384][i]
    assert s["status"] == pkg.CPS_OK and s["count"] == m["count"] <= cp_cap and s["out_len"] == len(plain)
    del out
    cnt = int(s["count"])
    ranges = [(70000, 71000), (len(plain) - 10, len(plain)), (0, 40000)]
    r = torch.tensor(np.array(ranges, np.int64), device=eng.dev)
    rc, offs, st, out_len, decoded, dst = eng.checkpoint_read_ranges(src, len(stream), cbit[0, :cnt + 1].contiguous(), uoff[0, :cnt + 1].contiguous(),
                                                                     windows[0, :cnt].contiguous(), r)
    torch.cuda.synchronize(eng.dev)
    assert rc == 0 and st.cpu().tolist() == [0, 0, 0] and decoded < cnt
    assert dst.cpu().numpy()[:out_len].tobytes() == b"".join(plain[b:e] for b, e in ranges)
