"""GPU tests of the one-pass index build (include/nxz_engine.h: nxz_batch_checkpoint_build; the kernel in
power-gzip_amd/csrc/nxz_checkpoint_build.hip): the batch of tests/test_gpu_checkpoints_fine.py -- raw, zlib and gzip streams of
100-250 KiB of plain bytes each -- and two hand-built streams with matches at the far edge of the window
(tests/checkpoint_build_cases.py), indexed with dst = NULL in every job.  Positions, states and records against the models
(tests/checkpoint_fine_model.py, tests/checkpoint_model.py) and against the existing index call on decoded output; every window
slot byte for byte against the plain bytes, the fill pattern everywhere else; then ranges read through what the build call wrote."""
import bisect
import errno
import importlib
import os
import random

import numpy as np
import pytest

import checkpoint_build_cases as B
import checkpoint_fine_model as F
import checkpoint_model as M

pytestmark = pytest.mark.gpu
pkg = importlib.import_module("power-gzip_amd")
KNOBS = ("NXZ_INFLATE_LANES_MIN", "NXZ_INFLATE_CUT", "NXZ_INFLATE_WG", "NXZ_INFLATE_WG_MAX", "NXZ_WG_PMIN", "NXZ_INFLATE_ORDER",
         "NXZ_BGZF_CHUNK", "NXZ_STREAMS_CHUNK")
W = F.WINDOW
PATTERN = 0xA5
SPANS = (4096, 32768, 65536, 1 << 20)
SMALL = ("far_fixed", "far_stored", "rle_zeros", "alice6_raw")           # the streams that are indexed with span 258
COARSE = (1, 4096, 65536)
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


def coarse(stream, fmt, span):
    m = M.index(stream, fmt, span)
    if m is not None:
        m = dict(m, hdr_len=F.header_len(stream, fmt), state=None)
    return m


class Batch:
    """the streams on the device at odd addresses, the models, and -- for the comparison with the existing call alone -- a target
    slot per stream that holds its decoded output"""

    def __init__(self, eng, pick=None, parent=None):
        import torch
        if parent is not None:                                            # a part of the batch as a batch of its own
            self.__dict__.update(parent.__dict__)
            for f in ("names", "fmt", "stream", "plain", "sat", "dat", "cap"):
                setattr(self, f, [getattr(parent, f)[i] for i in pick])
            self.model = {key: [v[i] for i in pick] for key, v in parent.model.items()}
            self.n = len(pick)
            return
        s = list(F.streams())
        text = s[0][3]
        s.insert(9, ("engine", F.FMT_ZLIB, engine_stream(eng, text), text))
        s += B.streams()
        self.names, self.fmt, self.stream, self.plain = ([x[k] for x in s] for k in range(4))
        self.n, self.eng = len(s), eng
        self.model = {span: [F.index(st, f, span) for st, f in zip(self.stream, self.fmt)] for span in SPANS}
        self.model[258] = [F.index(st, f, 258) if name in SMALL else None for name, st, f in zip(self.names, self.stream, self.fmt)]
        for span in COARSE:
            self.model[("coarse", span)] = [coarse(st, f, span) for st, f in zip(self.stream, self.fmt)]
        for span in SPANS:
            for i, m in enumerate(self.model[span]):
                assert (m is None) == (self.plain[i] is None) and (m is None or m["out_len"] == len(self.plain[i])), self.names[i]
        self.sat, pos = [], 0
        for i, st in enumerate(self.stream):                              # src at any alignment: 16 k + 1, + 2, ...
            pos = ((pos + 15) & ~15) + (i + 1) % 16
            self.sat.append(pos)
            pos += len(st)
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
        self.dst = torch.from_numpy(hd).to(eng.dev)

    def jobs(self, dst=None, repeat=1, **fields):
        j = np.zeros(self.n, pkg.JOB_DTYPE)
        for i in range(self.n):
            j[i]["src"] = self.src.data_ptr() + self.sat[i]
            j[i]["src_len"] = len(self.stream[i])
            j[i]["dst"] = 0 if dst is None else dst.data_ptr() + self.dat[i]
            j[i]["dst_cap"] = 0 if dst is None else self.cap[i]
            j[i]["in_adler"] = 1
        for k, v in fields.items():
            j[k] = v
        return self.eng.to_device(np.tile(j, repeat))

    def filled(self, n, cp_cap, shift=0):
        import torch
        dev = self.eng.dev
        wbuf = torch.full((n * cp_cap * W + 16,), PATTERN, dtype=torch.uint8, device=dev)
        return (torch.full((n, cp_cap + 1), -1, dtype=torch.int64, device=dev), torch.full((n, cp_cap + 1), -1, dtype=torch.int64, device=dev),
                torch.full((n, (cp_cap + 1) * STATE.itemsize), PATTERN, dtype=torch.uint8, device=dev),
                wbuf[shift:shift + n * cp_cap * W].view(n, cp_cap, W))

    def build(self, fmt, span, cp_cap, state=True, repeat=1, shift=0, **fields):
        """dst = 0 and dst_cap = 0 in every job; shift: the windows' first byte, from a 16-byte boundary"""
        eng, n = self.eng, self.n * repeat
        cbit, uoff, sta, windows = self.filled(n, cp_cap, shift)
        rc, cbit, uoff, sta, windows, streams = eng.checkpoint_build(fmt, self.jobs(None, repeat, **fields), n, span, cp_cap, sta if state else None,
                                                                     cbit, uoff, windows)
        assert rc == 0
        st = eng.results_to_host(streams, pkg.CHECKPOINT_STREAM_DTYPE)[:n]
        return cbit, uoff, sta, windows, st


@pytest.fixture(scope="module")
def batch(eng):
    return Batch(eng)


@pytest.fixture(scope="module")
def halves(batch):
    """the raw streams and the framed ones as batches of their own (raw streams have no header to tell them by)"""
    raw = [i for i in range(batch.n) if batch.fmt[i] == F.FMT_RAW]
    framed = [i for i in range(batch.n) if batch.fmt[i] != F.FMT_RAW]
    assert len(raw) == 6 and len(framed) == 9
    return ((Batch(None, raw, batch), pkg.engine.FMT_RAW), (Batch(None, framed, batch), pkg.FMT_AUTO))


def states_of(state_row):
    return [tuple(int(x) for x in s) for s in state_row.view(STATE)]


def check_positions(sub, key, cp_cap, cbit, uoff, state, st):
    """streams[], cbit, uoff and state against the model; entries behind what a stream stores still hold the fill"""
    cb, uo = cbit.cpu().numpy(), uoff.cpu().numpy()
    sta = state.cpu().numpy() if state is not None else None
    for i, m in enumerate(sub.model[key]):
        name, s = sub.names[i], st[i]
        if m is None:
            assert s["status"] == pkg.CPS_STREAM_FAILED and s["count"] == 0 and s["cc"] != 0 and s["out_len"] == 0, (name, s)
            assert (s["frame_status"], s["cc"] == 3) == ((pkg.FRAME_TRUNCATED, True) if name == "truncated" else (pkg.FRAME_DEFLATE, False)), (name, s)
            continue
        exp = pkg.CPS_MORE if m["count"] > cp_cap else pkg.CPS_OK
        assert (s["status"], s["count"], s["out_len"], s["cc"], s["frame_status"]) == (exp, m["count"], m["out_len"], 0, pkg.FRAME_OK), (name, key, s, m["count"])
        assert s["format"] == sub.fmt[i] and s["hdr_len"] == m["hdr_len"], (name, s)
        k = min(m["count"], cp_cap) + (0 if exp == pkg.CPS_MORE else 1)     # (with the sentinel, unless checkpoints were only counted)
        assert cb[i, :k].tolist() == m["cbit"][:k] and uo[i, :k].tolist() == m["uoff"][:k], (name, key)
        assert (cb[i, k:] == -1).all() and (uo[i, k:] == -1).all(), (name, key)
        if sta is None:
            continue
        if m["state"] is None:                                            # no state array was passed: this one is the test's own, untouched
            assert (sta[i] == PATTERN).all(), (name, key)
            continue
        assert states_of(sta[i, :k * 16]) == (m["state"][:k] if exp == pkg.CPS_MORE else m["state"][:k - 1] + [(0, 0, 0)]), (name, key)
        assert (sta[i, k * 16:] == PATTERN).all(), (name, key)


def check_windows(sub, key, cp_cap, windows, skip=()):
    """the first min(u, 32768) bytes of every stored slot are the bytes in front of u; everything else in the slots of streams that
    succeed is the fill (the slots of a stream that fails are its own to spoil)"""
    w = windows.cpu().numpy()
    for i, m in enumerate(sub.model[key]):
        if m is None or i in skip:
            continue
        stored = min(m["count"], cp_cap)
        want = np.full((cp_cap, W), PATTERN, np.uint8)
        plain = np.frombuffer(sub.plain[i], np.uint8)
        for k in range(stored):
            u = m["uoff"][k]
            n = min(u, W)
            want[k, :n] = plain[u - n:u]
        bad = np.nonzero((w[i] != want).any(axis=1))[0]
        assert bad.size == 0, (sub.names[i], key, "slots", bad[:8].tolist(), [m["uoff"][k] for k in bad[:8] if k < stored])


def test_the_batch_is_what_the_issue_asks_for(batch):
    assert batch.n == 15 and all(p is None or 100 << 10 <= len(p) <= 250 << 10 for p in batch.plain)
    assert batch.names == ["alice6_raw", "alice6_zlib", "alice6_gzip_fields", "alice1", "fixed_one_block", "rle_zeros", "stored", "mem9", "mem1",
                           "engine", "empty_final_block", "truncated", "bad_table", "far_fixed", "far_stored"]
    assert all((m is not None) == (n in SMALL) for n, m in zip(batch.names, batch.model[258]))
    assert all(m["count"] >= 450 for m in batch.model[258] if m is not None)        # hundreds of slots a stream
    assert all(3 <= len(p) // W <= 7 for p in batch.plain if p is not None)        # the ring wraps three to seven times
    j = batch.jobs().cpu().numpy().view(pkg.JOB_DTYPE)
    assert (j["dst"] == 0).all() and (j["dst_cap"] == 0).all() and len({int(a) % 16 for a in j["src"]}) >= 12


@pytest.mark.parametrize("span", SPANS)
def test_positions_states_and_windows_equal_the_model(halves, span):
    for sub, fmt in halves:
        cp_cap = max(m["count"] for m in sub.model[span] if m is not None) + 1
        cbit, uoff, state, wins, st = sub.build(fmt, span, cp_cap)
        check_positions(sub, span, cp_cap, cbit, uoff, state, st)
        check_windows(sub, span, cp_cap, wins)


def test_span_258_a_thousand_slots_a_stream(halves):
    for sub, fmt in halves:
        pick = [i for i in range(sub.n) if sub.names[i] in SMALL]
        part = Batch(None, pick, sub)
        cp_cap = max(m["count"] for m in part.model[258]) + 1
        cbit, uoff, state, wins, st = part.build(fmt, 258, cp_cap)
        check_positions(part, 258, cp_cap, cbit, uoff, state, st)
        check_windows(part, 258, cp_cap, wins)


@pytest.mark.parametrize("span", COARSE)
def test_without_states_the_checkpoints_are_the_coarse_index(halves, span):
    for sub, fmt in halves:
        key = ("coarse", span)
        cp_cap = max(m["count"] for m in sub.model[key] if m is not None) + 1
        cbit, uoff, state, wins, st = sub.build(fmt, span, cp_cap, state=False)
        check_positions(sub, key, cp_cap, cbit, uoff, state, st)
        check_windows(sub, key, cp_cap, wins)


def test_windows_at_any_alignment(halves):
    """slots that are not 16-byte aligned take the byte stores: the same bytes"""
    sub, fmt = halves[0]
    cp_cap = max(m["count"] for m in sub.model[32768] if m is not None) + 1
    for shift in (1, 7):
        cbit, uoff, state, wins, st = sub.build(fmt, 32768, cp_cap, shift=shift)
        assert wins.data_ptr() % 16 == shift
        check_positions(sub, 32768, cp_cap, cbit, uoff, state, st)
        check_windows(sub, 32768, cp_cap, wins)


def test_the_arrays_equal_the_existing_call_on_decoded_output(eng, halves):
    import torch
    for sub, fmt in halves:
        cp_cap = max(m["count"] for m in sub.model[4096] if m is not None) + 1
        n = sub.n
        for with_state in (True, False):
            cbit, uoff, state, wins, st = sub.build(fmt, 4096, cp_cap, state=with_state)
            c2, u2, s2, w2 = sub.filled(n, cp_cap)
            if with_state:
                rc, c2, u2, s2, w2, streams = eng.checkpoint_index_fine(fmt, sub.jobs(sub.dst), n, 4096, cp_cap, w2, c2, u2, s2)
            else:
                rc, c2, u2, w2, streams = eng.checkpoint_index(fmt, sub.jobs(sub.dst), n, 4096, cp_cap, w2, c2, u2)
            st2 = eng.results_to_host(streams, pkg.CHECKPOINT_STREAM_DTYPE)[:n]
            assert rc == 0
            ok = [i for i in range(n) if sub.plain[i] is not None]
            for f in st.dtype.names:
                assert (st[f] == st2[f]).all(), (f, st[f], st2[f])
            assert torch.equal(cbit[ok], c2[ok]) and torch.equal(uoff[ok], u2[ok]) and (not with_state or torch.equal(state[ok], s2[ok]))
            assert torch.equal(wins[ok], w2[ok])                          # (up to w: the bytes; behind it: the fill, in both)
            assert sum(int(s["count"]) for s in st) > (6 * n if with_state else n)          # (checkpoints inside blocks; block headers alone)


def test_a_small_cap_counts_on(halves):
    for sub, fmt in halves:
        cp_cap = sub.model[4096][0]["count"] - 1
        assert cp_cap >= 2
        cbit, uoff, state, wins, st = sub.build(fmt, 4096, cp_cap)
        assert st[0]["status"] == pkg.CPS_MORE and st[0]["count"] == cp_cap + 1
        assert sum(1 for s in st if s["status"] == pkg.CPS_MORE) >= 2
        check_positions(sub, 4096, cp_cap, cbit, uoff, state, st)         # (no sentinel: the entry at [cp_cap] is the fill)
        check_windows(sub, 4096, cp_cap, wins)


def test_failing_streams_fail_as_in_the_index_calls_and_touch_nothing_else(eng, halves):
    sub, fmt = halves[1]
    bad = [sub.names.index("truncated"), sub.names.index("bad_table")]
    cp_cap = 40
    cbit, uoff, state, wins, st = sub.build(fmt, 4096, cp_cap)
    rc, _, _, _, _, streams = eng.checkpoint_index_fine(fmt, sub.jobs(), sub.n, 4096, cp_cap)
    ref = eng.results_to_host(streams, pkg.CHECKPOINT_STREAM_DTYPE)
    assert rc == 0
    for i in bad:
        assert st[i] == ref[i] and st[i]["status"] == pkg.CPS_STREAM_FAILED and st[i]["count"] == 0, (sub.names[i], st[i], ref[i])
    assert (st[bad[0]]["cc"], st[bad[0]]["frame_status"]) == (3, pkg.FRAME_TRUNCATED) and st[bad[1]]["frame_status"] == pkg.FRAME_DEFLATE
    # the truncated stream passed checkpoints before it failed: its own slots may hold bytes, its neighbours' hold theirs and the fill
    check_positions(sub, 4096, cp_cap, cbit, uoff, state, st)
    check_windows(sub, 4096, cp_cap, wins)
    assert bad == [sub.n - 2, sub.n - 1] and sub.plain[bad[0] - 1] is not None


def test_refusals(eng, halves):
    sub, fmt = halves[1]
    for field, value in (("hist_len", 16), ("resume", 3 << 20)):
        v = np.zeros(sub.n, np.uint32)
        v[1] = value
        cbit, uoff, state, wins, st = sub.build(fmt, 4096, 64, **{field: v})
        assert st[1]["status"] == pkg.CPS_INVALID and st[1]["count"] == 0 and st[1]["out_len"] == 0
        assert (cbit[1] == -1).all() and bool((wins[1] == PATTERN).all()) and st[0]["status"] == pkg.CPS_OK and st[2]["status"] == pkg.CPS_OK
        check_windows(sub, 4096, 64, wins, skip=(1,))
    jobs = sub.jobs()
    good = (fmt, jobs, sub.n, 4096, 16)
    assert eng.checkpoint_build(*good)[0] == 0
    for args in ((fmt, jobs, sub.n, 257, 16), (fmt, jobs, sub.n, 0, 16), (fmt, jobs, sub.n, 4096, 0), (7, jobs, sub.n, 4096, 16), (-1, jobs, sub.n, 4096, 16),
                 (fmt, None, sub.n, 4096, 16)):
        assert eng.checkpoint_build(*args)[0] == -errno.EINVAL, args[2:]
    assert eng.checkpoint_build(fmt, jobs, sub.n, 0, 16, state=False)[0] == -errno.EINVAL          # span == 0: without states too
    assert eng.checkpoint_build(fmt, jobs, sub.n, 257, 16, state=False)[0] == 0                    # span < 258: with states only
    L, h = eng.L, eng.stream_handle()
    c, u, s, w = sub.filled(sub.n, 16)
    streams = eng.torch.zeros(sub.n * 32, dtype=eng.torch.uint8, device=eng.dev)
    ptrs = [c.data_ptr(), u.data_ptr(), s.data_ptr(), w.data_ptr(), streams.data_ptr()]
    assert L.nxz_batch_checkpoint_build(eng.ctx, fmt, jobs.data_ptr(), sub.n, 4096, 16, *ptrs, h) == 0
    for k in (0, 1, 3, 4):                                                # cbit, uoff, windows, streams: required (state: NULL has a meaning)
        p = list(ptrs)
        p[k] = None
        assert L.nxz_batch_checkpoint_build(eng.ctx, fmt, jobs.data_ptr(), sub.n, 4096, 16, *p, h) == -errno.EINVAL, k
    assert L.nxz_batch_checkpoint_build(eng.ctx, fmt, jobs.data_ptr(), 1 << 31, 4096, 16, *ptrs, h) == -errno.EINVAL
    assert L.nxz_batch_checkpoint_build(None, fmt, jobs.data_ptr(), sub.n, 4096, 16, *ptrs, h) == -errno.EINVAL
    assert L.nxz_batch_checkpoint_build(eng.ctx, fmt, None, 0, 4096, 16, None, None, None, None, None, h) == 0       # n == 0
    assert eng.checkpoint_build(fmt, None, 0, 4096, 16)[0] == 0


def test_a_second_build_call_allocates_nothing(eng, halves):
    """135 jobs: the long ones first, the order in the stream's scratch -- which the second call finds as it is"""
    import torch
    sub, fmt = halves[1]
    first = sub.build(fmt, 65536, 8, repeat=15)
    torch.cuda.synchronize(eng.dev)
    jobs = sub.jobs(repeat=15)
    cbit, uoff, state, wins = sub.filled(sub.n * 15, 8)
    streams = torch.zeros(sub.n * 15 * 32, dtype=torch.uint8, device=eng.dev)
    torch.cuda.synchronize(eng.dev)
    free0 = torch.cuda.mem_get_info(eng.dev)[0]
    rc = eng.checkpoint_build(fmt, jobs, sub.n * 15, 65536, 8, state, cbit, uoff, wins, streams)[0]
    torch.cuda.synchronize(eng.dev)
    assert rc == 0 and torch.cuda.mem_get_info(eng.dev)[0] == free0
    ok = [i for i in range(sub.n * 15) if sub.plain[i % sub.n] is not None]
    assert torch.equal(cbit, first[0]) and torch.equal(uoff, first[1]) and torch.equal(state, first[2]) and torch.equal(wins[ok], first[3][ok])
    st = eng.results_to_host(streams, pkg.CHECKPOINT_STREAM_DTYPE)
    assert (st == first[4]).all() and sum(1 for s in st if s["status"] == pkg.CPS_OK) == 15 * 7


# ---- end to end: ranges through what the build call wrote -------------------------------------------------------------------------
def segments_of(m, ranges):
    u, L, out = m["uoff"], m["count"], set()
    for b, e in ranges:
        if b < e <= u[L]:
            out |= set(range(bisect.bisect_right(u[:L], b) - 1, bisect.bisect_right(u[:L], e - 1)))
    return out


@pytest.mark.parametrize("name,span", [("far_fixed", 4096), ("far_stored", 4096), ("mem9", 32768), ("stored", 4096), ("far_fixed", 258)])
def test_ranges_through_a_built_index_equal_the_plain_slices(eng, halves, name, span):
    import torch
    sub, fmt = halves[0] if name in halves[0][0].names else halves[1]
    k = sub.names.index(name)
    part = Batch(None, [k], sub)
    m, plain, length = part.model[span][0], part.plain[0], len(part.stream[0])
    cbit, uoff, state, wins, st = part.build(fmt, span, m["count"])
    assert st[0]["status"] == pkg.CPS_OK and st[0]["count"] == m["count"]
    src = sub.src[sub.sat[k]:sub.sat[k] + length].clone()
    n = m["out_len"]
    rnd = random.Random(len(name) + span)
    ranges = [(0, n), (n - 1, n), (0, 1), (7, 7), (W - 1, W + 1), (2 * W - 100, 2 * W + 100), (n - 5, n + 1)]
    ranges += [(b, min(n, b + rnd.choice([1, 100, 20000]))) for b in (rnd.randrange(n) for _ in range(40))]
    ranges += [(m["uoff"][j] - 1, m["uoff"][j] + 1) for j in rnd.sample(range(1, m["count"]), min(10, m["count"] - 1))]
    r = torch.tensor(np.array(ranges, np.int64), device=eng.dev)
    rc, offs, status, out_len, decoded, dst = eng.checkpoint_read_ranges_fine(src, length, cbit[0].contiguous(), uoff[0].contiguous(),
                                                                              state[0].contiguous(), wins[0].contiguous(), r)
    torch.cuda.synchronize(eng.dev)
    offs, status, got = offs.cpu().numpy(), status.cpu().numpy(), dst.cpu().numpy()
    assert rc == 0 and decoded == len(segments_of(m, ranges)) == m["count"]
    for j, (b, e) in enumerate(ranges):
        bad = not (b <= e <= n)
        assert status[j] == (pkg.RANGE_OUT_OF_BOUNDS if bad else pkg.RANGE_OK), (j, b, e)
        assert got[offs[j]:offs[j + 1]].tobytes() == (b"" if bad else plain[b:e]), (j, b, e)
    assert out_len == sum(e - b for b, e in ranges if b <= e <= n)
