"""GPU tests of nxz_batch_deflate_streams_indexed (include/nxz_engine.h; the kernels in power-gzip_amd/csrc/nxz_streams_index.hip, the
rules in nxz_streams_index.h): nxz_batch_deflate_streams that writes the checkpoint index of its streams on the way.  The yardsticks:
nxz_batch_deflate_streams for the streams and the results (byte for byte), nxz_batch_checkpoint_index run on the finished streams with
dst = the source for every row of the index (positions, records, windows), tests/checkpoint_model.py (zlib's inflate with Z_BLOCK)
for a subset, and the source's own bytes for ranges read back through nxz_batch_checkpoint_read_ranges.  Every array the call writes
to is filled with a canary first: what it must not write is checked as well."""
import errno
import importlib
import os

import numpy as np
import pytest

import checkpoint_model as M
from datagen import make_block

pytestmark = pytest.mark.gpu
pkg = importlib.import_module("power-gzip_amd")
RAW, ZLIB, GZIP = pkg.engine.FMT_RAW, pkg.engine.FMT_ZLIB, pkg.engine.FMT_GZIP
SJ, SR, CS, JOB = pkg.engine.STREAM_JOB_DTYPE, pkg.engine.STREAM_RESULT_DTYPE, pkg.CHECKPOINT_STREAM_DTYPE, pkg.JOB_DTYPE
FHT, DHTGEN = pkg.FC_COMPRESS_FHT, pkg.FC_COMPRESS_DHTGEN
W = pkg.CHECKPOINT_WINDOW
HDR_LEN = {RAW: 0, ZLIB: 2, GZIP: 10}
CANARY, TAIL = 0xc3, 64
CANARY64 = int(np.frombuffer(bytes([CANARY]) * 8, "<i8")[0])
KNOBS = ("NXZ_STREAMS_CHUNK", "NXZ_BGZF_CHUNK", "NXZ_INFLATE_LANES_MIN", "NXZ_INFLATE_CUT", "NXZ_INFLATE_WG", "NXZ_INFLATE_ORDER")


@pytest.fixture(scope="module")
def eng():
    saved = {k: os.environ.pop(k, None) for k in KNOBS}
    e = pkg.Engine(0)
    yield e
    e.close()
    for k, v in saved.items():
        if v is not None:
            os.environ[k] = v


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


_bufs = {}


def buffers(hist_max):
    """edge_buffers() of tests/test_gpu_streams.py restated, and random bytes of exactly 65536: at hist_max 0 one stored piece of two blocks"""
    if hist_max not in _bufs:
        B = block_bytes(hist_max)
        _bufs[hist_max] = [b"", make_block("alice", 1, 1), make_block("lz", 15, 2), make_block("zeros", 16, 3), make_block("alice", B - 1, 4),
                           make_block("random", B, 5), make_block("lz", B + 1, 6), mixed(2 * B, 7), mixed(2 * B + 17, 8), mixed(65 * B + 5, 9),
                           make_block("random", 65536, 10)]
        assert [len(b) for b in _bufs[hist_max][:10]] == [0, 1, 15, 16, B - 1, B, B + 1, 2 * B, 2 * B + 17, 65 * B + 5]
    return _bufs[hist_max]


class Layout:
    """sources at 16-byte aligned offsets of one device buffer (src_off moves one off them), targets in slots of one buffer of canary bytes"""

    def __init__(self, eng, fmt, bufs, hist_max, cap_delta=None, src_off=None):
        import torch
        n = self.n = len(bufs)
        self.eng, self.fmt, self.bufs, self.hist_max = eng, fmt, bufs, hist_max
        cap_delta, src_off = cap_delta or [0] * n, src_off or [0] * n
        self.cap = [eng.deflate_stream_bound(len(b), hist_max, fmt) + d for b, d in zip(bufs, cap_delta)]
        self.sat, pos = [], 0
        for b, o in zip(bufs, src_off):
            self.sat.append(pos + o)
            pos += (o + len(b) + 31) & ~15
        hs = np.zeros(pos + 16, np.uint8)
        for b, a in zip(bufs, self.sat):
            hs[a:a + len(b)] = np.frombuffer(b, np.uint8)
        self.dat, pos = [], 0
        for c in self.cap:
            self.dat.append(pos + 16)
            pos += (16 + c + TAIL + 15) & ~15
        self.dst_bytes = pos + 16
        self.src = torch.from_numpy(hs).to(eng.dev)

    def jobs(self, dst):
        j = np.zeros(self.n, SJ)
        for i in range(self.n):
            j[i] = (self.src.data_ptr() + self.sat[i], dst.data_ptr() + self.dat[i], len(self.bufs[i]), self.cap[i])
        return j

    def fresh_dst(self):
        import torch
        return torch.full((self.dst_bytes,), CANARY, dtype=torch.uint8, device=self.eng.dev)


class Rows:
    """the index arrays of one call, each with a canary row (or slot) in front and behind"""

    def __init__(self, eng, n, cp_cap, windows=True):
        import torch
        t, dev = torch, eng.dev
        self.n, self.cp_cap = n, cp_cap
        self.cbit_all = t.full((n + 2, cp_cap + 1), CANARY64, dtype=t.int64, device=dev)
        self.uoff_all = t.full((n + 2, cp_cap + 1), CANARY64, dtype=t.int64, device=dev)
        self.st_all = t.full(((n + 2) * CS.itemsize,), CANARY, dtype=t.uint8, device=dev)
        self.win_all = t.full((n * cp_cap + 2, W), CANARY, dtype=t.uint8, device=dev) if windows else None
        self.cbit, self.uoff = self.cbit_all[1:n + 1], self.uoff_all[1:n + 1]
        self.streams = self.st_all[CS.itemsize:(n + 1) * CS.itemsize]
        self.windows = self.win_all[1:n * cp_cap + 1].view(n, cp_cap, W) if windows else None

    def host(self, eng):
        import torch
        torch.cuda.synchronize(eng.dev)
        self.h_cbit, self.h_uoff = self.cbit_all.cpu().numpy(), self.uoff_all.cpu().numpy()
        self.h_st = self.st_all.cpu().numpy()
        self.st = self.h_st[CS.itemsize:(self.n + 1) * CS.itemsize].view(CS).copy()
        return self

    def guards_hold(self):
        ok = (self.h_cbit[[0, -1]] == CANARY64).all() and (self.h_uoff[[0, -1]] == CANARY64).all()
        ok = ok and (self.h_st[:CS.itemsize] == CANARY).all() and (self.h_st[-CS.itemsize:] == CANARY).all()
        if self.win_all is not None:
            ok = ok and bool((self.win_all[0] == CANARY).all()) and bool((self.win_all[-1] == CANARY).all())
        return bool(ok)

    def window_image(self):
        """what the slots must hold given the stored positions, on the device: the first min(uoff, 32768) bytes unknown (-1), the rest
        and every unstored slot the canary -> (mask of window bytes, the slots)"""
        import torch
        cnt = torch.from_numpy(np.minimum(self.st["count"], self.cp_cap).astype(np.int64)).to(self.windows.device)
        k = torch.arange(self.cp_cap, device=self.windows.device)
        stored = k[None, :] < cnt[:, None]
        w = torch.where(stored, torch.clamp(self.uoff[:, :self.cp_cap], max=W), torch.zeros_like(self.uoff[:, :self.cp_cap]))
        return torch.arange(W, device=self.windows.device)[None, None, :] < w[:, :, None]


def run_plain(eng, lay, fc, level=-1):
    dst = lay.fresh_dst()
    rc, res = eng.deflate_stream_jobs(fc, lay.fmt, lay.jobs(dst), hist_max=lay.hist_max, level=level)
    assert rc == 0
    return dst, eng.results_to_host(res, SR)[:lay.n].copy()


def run_indexed(eng, lay, fc, span, cp_cap, windows=True, index_jobs=True, level=-1):
    import torch
    dst = lay.fresh_dst()
    rows = Rows(eng, lay.n, cp_cap, windows)
    ij = torch.full(((lay.n + 2) * JOB.itemsize,), CANARY, dtype=torch.uint8, device=eng.dev) if index_jobs else None
    rc, res, _, _, _, _, _ = eng.deflate_stream_jobs_indexed(fc, lay.fmt, lay.jobs(dst), span, cp_cap, windows=rows.windows if windows else False,
                                                             index_jobs=ij[JOB.itemsize:(lay.n + 1) * JOB.itemsize] if index_jobs else False,
                                                             hist_max=lay.hist_max, level=level, cbit=rows.cbit, uoff=rows.uoff, streams=rows.streams)
    assert rc == 0
    rows.host(eng)
    rows.dst, rows.res = dst, eng.results_to_host(res, SR)[:lay.n].copy()
    if index_jobs:
        h = ij.cpu().numpy()
        assert (h[:JOB.itemsize] == CANARY).all() and (h[-JOB.itemsize:] == CANARY).all()
        rows.ij_dev = ij[JOB.itemsize:(lay.n + 1) * JOB.itemsize]
        rows.ij = h[JOB.itemsize:(lay.n + 1) * JOB.itemsize].view(JOB).copy()
    return rows


def run_reference(eng, lay, dst, res, span, cp_cap, which=None, windows=True):
    """nxz_batch_checkpoint_index on the finished streams `which` (all by default), dst = the source"""
    which = list(range(lay.n)) if which is None else which
    j = np.zeros(len(which), JOB)
    for r, i in enumerate(which):
        j[r]["src"], j[r]["src_len"] = dst.data_ptr() + lay.dat[i], res["out_len"][i]
        j[r]["dst"], j[r]["dst_cap"] = lay.src.data_ptr() + lay.sat[i], len(lay.bufs[i])
        j[r]["in_adler"] = 1
    rows = Rows(eng, len(which), cp_cap, windows)
    rc = eng.checkpoint_index(lay.fmt, eng.to_device(j), len(which), span, cp_cap, windows=rows.windows if windows else False, cbit=rows.cbit,
                              uoff=rows.uoff, streams=rows.streams)[0]
    assert rc == 0
    return rows.host(eng)


def same_rows(got, ref, rows_got=None, rows_ref=None, windows=True):
    """rows rows_got of `got` are rows rows_ref of `ref`: positions up to the sentinel, the record, the windows; the canary everywhere else"""
    import torch
    rows_got = list(range(got.n)) if rows_got is None else rows_got
    rows_ref = list(range(ref.n)) if rows_ref is None else rows_ref
    cap = got.cp_cap
    for a, b in zip(rows_got, rows_ref):
        s, r = got.st[a], ref.st[b]
        assert s.tobytes() == r.tobytes(), (a, s, r)
        assert s["status"] == (pkg.CPS_MORE if s["count"] > cap else pkg.CPS_OK), (a, s)
        written = int(s["count"]) + 1 if s["count"] <= cap else cap          # (with the sentinel, or the stored ones alone)
        for x, y in ((got.h_cbit, ref.h_cbit), (got.h_uoff, ref.h_uoff)):
            assert np.array_equal(x[1 + a, :written], y[1 + b, :written]), (a, x[1 + a, :written], y[1 + b, :written])
            assert (x[1 + a, written:] == CANARY64).all(), (a, "written behind the row's entries")
    assert got.guards_hold()
    if windows:
        mask = got.window_image()
        assert bool((got.windows[~mask] == CANARY).all()), "a window slot written behind its window, or an unstored slot written"
        ia, ib = torch.tensor(rows_got, device=mask.device), torch.tensor(rows_ref, device=mask.device)
        mg, mr = mask[ia], ref.window_image()[ib]
        assert bool((mg == mr).all())
        assert bool((got.windows[ia][mg] == ref.windows[ib][mr]).all()), "a window differs from the index call's"


def longest_count(rows):
    return int(rows.st["count"].max())


@pytest.mark.parametrize("fmt", [RAW, ZLIB, GZIP])
@pytest.mark.parametrize("fc", [FHT, DHTGEN])
@pytest.mark.parametrize("hist_max", [0, 4096, 32768])
def test_rows_are_the_index_calls(eng, fmt, fc, hist_max):
    import torch
    B = block_bytes(hist_max)
    bufs = buffers(hist_max)
    lay = Layout(eng, fmt, bufs, hist_max)
    pdst, pres = run_plain(eng, lay, fc)
    assert (pres["cc"] == 0).all()
    pout = pdst.cpu().numpy()
    full = 2 * 65 + 2                                        # two headers a block at most, and room for the sentinel
    kept = {}
    for span in (1, B, B + 1, 3 * B, 2 ** 40):
        got = run_indexed(eng, lay, fc, span, full)
        # the streams and the results are the plain call's
        assert got.res.tobytes() == pres.tobytes() and np.array_equal(got.dst.cpu().numpy(), pout), span
        ref = run_reference(eng, lay, got.dst, got.res, span, full)
        same_rows(got, ref)
        assert (got.st["status"] == pkg.CPS_OK).all() and (got.st["format"] == fmt).all() and (got.st["hdr_len"] == HDR_LEN[fmt]).all()
        assert list(got.st["out_len"]) == [len(b) for b in bufs]
        assert (got.h_cbit[1:-1, 0] == 8 * HDR_LEN[fmt]).all() and (got.h_uoff[1:-1, 0] == 0).all()
        # the reader's jobs
        for i in range(lay.n):
            assert got.ij[i]["src"] == got.dst.data_ptr() + lay.dat[i] and got.ij[i]["src_len"] == got.res["out_len"][i] and got.ij[i]["in_adler"] == 1
            assert all(got.ij[i][f] == 0 for f in ("dst", "hist_len", "dst_cap", "in_crc", "dht_index", "resume", "reserved"))
        kept[span] = got
    assert list(kept[2 ** 40].st["count"]) == [1] * lay.n and kept[1].st["count"][9] >= 65
    # the set covers what it is meant to: a marker (a checkpoint inside a byte), a later checkpoint on a byte boundary, and -- where a
    # block carries 65536 bytes -- the second stored block of a stored piece
    marker = aligned = second = False
    for span, got in kept.items():
        for i in range(lay.n):
            c = int(got.st["count"][i])
            cb, uo = got.h_cbit[1 + i, 1:c], got.h_uoff[1 + i, 1:c]
            marker |= bool((cb % 8 != 0).any())
            aligned |= bool((cb % 8 == 0).any())
            second |= bool((uo % B == 65535).any())
    assert marker and aligned and (second or hist_max != 0), (marker, aligned, second)
    # cp_cap 1, exactly the longest stream's count, and one fewer: NXZ_CPS_MORE with the true count and no sentinel
    cnt = longest_count(kept[B])
    assert cnt >= 60
    for cap in (1, cnt, cnt - 1):
        got = run_indexed(eng, lay, fc, B, cap)
        same_rows(got, run_reference(eng, lay, got.dst, got.res, B, cap))
        assert list(got.st["count"]) == list(kept[B].st["count"])
        assert got.st["status"][9] == (pkg.CPS_OK if cap == cnt else pkg.CPS_MORE)
        assert np.array_equal(got.h_cbit[1:-1, :min(cap, 2)], kept[B].h_cbit[1:-1, :min(cap, 2)])
    # and back: ranges through the reader's jobs and the rows, with no host step in between (state NULL)
    got = kept[B]
    ranges = ranges_for(got, lay, B)
    q = np.zeros(len(ranges), pkg.BATCH_RANGE_DTYPE)
    for r, (job, b, e) in enumerate(ranges):
        q[r] = (job, 0, b, e)
    rc, offs, status, out_len, decoded, data = eng.checkpoint_read_ranges_batch(got.ij_dev, lay.n, full, got.cbit.contiguous(), got.uoff.contiguous(), None,
                                                                                got.windows.contiguous(), got.streams, eng.to_device(q))
    torch.cuda.synchronize(eng.dev)
    assert rc == 0 and (status.cpu().numpy() == pkg.RANGE_OK).all(), (rc, status)
    offs, data = offs.cpu().numpy(), data.cpu().numpy()
    for r, (job, b, e) in enumerate(ranges):
        assert data[offs[r]:offs[r + 1]].tobytes() == bufs[job][b:e], (job, b, e)


def ranges_for(got, lay, B):
    """(job, begin, end): one that straddles a checkpoint, one that ends at src_len, an empty one, and one that straddles a marker
    checkpoint (a segment that begins inside a byte) -- the test fails if the index has none"""
    out = []
    n9 = len(lay.bufs[9])
    u = got.h_uoff[1 + 9, :int(got.st["count"][9])]
    cb = got.h_cbit[1 + 9, :int(got.st["count"][9])]
    out.append((9, int(u[3]) - 1000, int(u[3]) + 1000))
    out.append((9, n9 - 70000, n9))
    out.append((9, 12345, 12345))
    inside = [k for k in range(1, len(cb)) if cb[k] % 8 != 0]
    assert inside, "no marker checkpoint in the long stream"
    k = inside[len(inside) // 2]
    out.append((9, max(int(u[k]) - 40000, 0), min(int(u[k]) + 40000, n9)))
    out.append((8, 0, len(lay.bufs[8])))
    out.append((1, 0, 1))
    out.append((0, 0, 0))
    return out


def test_rows_are_zlibs(eng):
    """gzip, exact tables, hist_max 0: the rows against zlib's own block boundaries (tests/checkpoint_model.py)"""
    B = 65536
    lay = Layout(eng, GZIP, buffers(0), 0)
    for span in (1, B, B + 1, 3 * B, 2 ** 40):
        got = run_indexed(eng, lay, DHTGEN, span, 132, windows=False)
        out = got.dst.cpu().numpy()
        for i, b in enumerate(lay.bufs):
            stream = out[lay.dat[i]:lay.dat[i] + int(got.res["out_len"][i])].tobytes()
            idx = M.index(stream, GZIP, span)
            assert idx is not None and idx["plain"] == b
            c = int(got.st["count"][i])
            assert c == idx["count"] and got.st["out_len"][i] == idx["out_len"], (span, i)
            assert list(got.h_cbit[1 + i, :c + 1]) == idx["cbit"] and list(got.h_uoff[1 + i, :c + 1]) == idx["uoff"], (span, i)


def test_chunks_do_not_show(eng, monkeypatch):
    hist_max = 4096
    B = block_bytes(hist_max)
    lay = Layout(eng, ZLIB, buffers(hist_max), hist_max)
    span = 5 * B // 2
    monkeypatch.delenv("NXZ_STREAMS_CHUNK", raising=False)
    base = run_indexed(eng, lay, DHTGEN, span, 40)
    assert base.st["count"][9] >= 20 and (base.st["status"] == pkg.CPS_OK).all()
    same_rows(base, run_reference(eng, lay, base.dst, base.res, span, 40))
    for chunk in (3, 1, 64):
        monkeypatch.setenv("NXZ_STREAMS_CHUNK", str(chunk))
        got = run_indexed(eng, lay, DHTGEN, span, 40)
        assert np.array_equal(got.h_cbit, base.h_cbit) and np.array_equal(got.h_uoff, base.h_uoff) and np.array_equal(got.h_st, base.h_st), chunk
        assert bool((got.win_all == base.win_all).all()) and bool((got.dst == base.dst).all()), chunk
        assert got.ij["src_len"].tolist() == base.ij["src_len"].tolist()


@pytest.mark.parametrize("how,cc", [("short", 13), ("misaligned", 8)])
def test_a_refused_stream_between_two_good_ones(eng, how, cc):
    B = 65536
    bufs = [mixed(3 * B + 100, 21), mixed(2 * B + 50, 22), mixed(4 * B, 23)]
    lay = Layout(eng, GZIP, bufs, 0, cap_delta=[0, -1 if how == "short" else 0, 0], src_off=[0, 8 if how == "misaligned" else 0, 0])
    got = run_indexed(eng, lay, DHTGEN, B, 12)
    assert list(got.res["cc"]) == [0, cc, 0]
    s = got.st[1]
    assert (s["status"], s["count"], s["cc"]) == (pkg.CPS_INVALID, 0, cc) and (s["format"], s["hdr_len"], s["out_len"], s["frame_status"]) == (0, 0, 0, 0)
    assert (got.h_cbit[2] == CANARY64).all() and (got.h_uoff[2] == CANARY64).all(), "the refused stream's row was written"
    assert bool((got.windows[1] == CANARY).all()), "the refused stream's slots were written"
    assert (got.ij[1]["src"], got.ij[1]["src_len"], got.ij[1]["dst"], got.ij[1]["in_adler"]) == (0, 0, 0, 1)
    # its target keeps the canary, the neighbours are what they are without it
    out = got.dst.cpu().numpy()
    assert (out[lay.dat[1] - 16:lay.dat[2] - 16] == CANARY).all()
    ref = run_reference(eng, lay, got.dst, got.res, B, 12, which=[0, 2])
    keep = got.st[1].copy()
    same_rows(got, ref, rows_got=[0, 2], rows_ref=[0, 1])
    assert got.st[1] == keep and got.st["count"][0] >= 4 and got.st["count"][2] >= 4


def test_positions_alone_and_no_reader_jobs(eng):
    hist_max = 32768
    B = block_bytes(hist_max)
    lay = Layout(eng, RAW, buffers(hist_max), hist_max)
    base = run_indexed(eng, lay, FHT, B, 140)
    got = run_indexed(eng, lay, FHT, B, 140, windows=False, index_jobs=False)
    assert (got.st["status"] == pkg.CPS_OK).all() and got.guards_hold()
    assert np.array_equal(got.h_cbit, base.h_cbit) and np.array_equal(got.h_uoff, base.h_uoff) and np.array_equal(got.h_st, base.h_st)
    assert got.res.tobytes() == base.res.tobytes() and bool((got.dst == base.dst).all())
    same_rows(got, run_reference(eng, lay, got.dst, got.res, B, 140, windows=False), windows=False)


def test_argument_errors(eng):
    import torch
    lay = Layout(eng, ZLIB, [make_block("alice", 1000, 1), make_block("lz", 2000, 2)], 0)
    dst = lay.fresh_dst()
    j = lay.jobs(dst)
    rows = Rows(eng, 2, 4)
    E = -errno.EINVAL

    def call(span=65536, cp_cap=4, jobs=j, **over):
        a = dict(cbit=rows.cbit, uoff=rows.uoff, streams=rows.streams, windows=rows.windows)
        a.update(over)
        return eng.deflate_stream_jobs_indexed(DHTGEN, ZLIB, jobs, span, cp_cap, index_jobs=False, **a)[0]
    assert call(span=0) == E and call(cp_cap=0) == E
    assert call(cbit=False) == E and call(uoff=False) == E and call(streams=False) == E
    assert call(cp_cap=2 ** 31) == E and call(cp_cap=2 ** 31 - 1, windows=False) == E         # 2 * (cp_cap + 1) >= 2^32
    assert call(jobs=j[:0]) == 0 and call(jobs=j[:0], cbit=False, uoff=False, streams=False, windows=False) == 0
    assert call(jobs=j[:0], span=0) == E
    # the plain call's refusals are still there
    assert eng.deflate_stream_jobs_indexed(pkg.FC_COMPRESS_DHT, ZLIB, j, 65536, 4, index_jobs=False, cbit=rows.cbit, uoff=rows.uoff, streams=rows.streams,
                                           windows=rows.windows)[0] == E
    torch.cuda.synchronize(eng.dev)
    # nothing was written by any of them ...
    rows.host(eng)
    assert (rows.h_cbit == CANARY64).all() and (rows.h_st == CANARY).all() and bool((rows.win_all == CANARY).all()) and bool((dst == CANARY).all())
    # ... and the call that is right works
    assert call() == 0
    rows.host(eng)
    assert list(rows.st["status"]) == [pkg.CPS_OK] * 2 and list(rows.st["count"]) == [1, 1]
