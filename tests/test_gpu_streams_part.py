"""GPU tests of nxz_batch_deflate_streams_part (include/nxz_engine.h; the kernels in power-gzip_amd/csrc/nxz_streams_part.hip, the rules
in nxz_streams_part.h): streams written in parts, a device buffer a part, the running state in a carry record on the device.  The
yardsticks are nxz_deflate_host_hist with final = LAST and prev = everything in front of the part -- the engine's own host-buffer
path, whose raw stream a part's deflate data must equal byte for byte --, zlib on the parts laid end to end and on every prefix of
them, zlib's crc32 / adler32 for the carry, the plain call nxz_batch_deflate_streams for a part that is a whole stream, and the
device's framed decoder."""
import ctypes as C
import errno
import importlib
import struct
import zlib

import numpy as np
import pytest

from datagen import make_block
from test_gpu_streams_dict import block_bytes, edge_buffers, jsonish, mixed

pytestmark = pytest.mark.gpu
pkg = importlib.import_module("power-gzip_amd")
E = pkg.engine
RAW, ZLIB, GZIP = E.FMT_RAW, E.FMT_ZLIB, E.FMT_GZIP
SJ, SR, PJ, CY = E.STREAM_JOB_DTYPE, E.STREAM_RESULT_DTYPE, E.STREAM_PART_JOB_DTYPE, E.STREAM_CARRY_DTYPE
FHT, DHTGEN = pkg.FC_COMPRESS_FHT, pkg.FC_COMPRESS_DHTGEN
FIRST, LAST = E.PART_FIRST, E.PART_LAST
WBITS = {RAW: -15, ZLIB: 15, GZIP: 31}
CANARY, TAIL = 0xc3, 64
INVALID_OP, TARGET_SPACE = 8, 13
FLG = {-1: 0x9c, 1: 0x01, 5: 0x5e, 6: 0x9c, 9: 0xda}             # zlib's FLG byte by level
GZ_HEADER = bytes.fromhex("1f8b0800000000000403")
PREV_KEEP = 32768 + 5                                            # what a caller keeps of the source in front: more than any window


@pytest.fixture(scope="module")
def eng():
    e = pkg.Engine(0)
    e.L.nxz_deflate_host_bound_hist.restype = C.c_size_t
    e.L.nxz_deflate_host_bound_hist.argtypes = [C.c_size_t, C.c_uint32]
    e.L.nxz_deflate_host_hist.argtypes = [C.c_void_p, C.c_int, C.c_char_p, C.c_size_t, C.c_int, C.c_uint32, C.c_char_p, C.c_size_t,
                                          C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    yield e
    e.close()


_ref = {}


def host_part(eng, fc, data, final, hist_max, prev):
    """the raw deflate data nxz_deflate_host_hist writes for `data` with `prev` as the earlier input -- the parent's code
    (only the tail of prev counts: the last PREV_KEEP bytes are handed over)"""
    prev = (prev or b"")[-PREV_KEEP:]
    key = (fc, hist_max, bool(final), hash(data), len(data), hash(prev), len(prev))
    if key not in _ref:
        if not data:
            _ref[key] = bytes.fromhex("010000ffff") if final else b""       # (the host call takes no empty buffer)
        else:
            cap = eng.L.nxz_deflate_host_bound_hist(len(data), hist_max)
            dst = C.create_string_buffer(cap)
            n, crc, adler = C.c_size_t(), C.c_uint32(), C.c_uint32()
            rc = eng.L.nxz_deflate_host_hist(eng.ctx, fc, data, len(data), 1 if final else 0, hist_max, prev if prev else None, len(prev),
                                             dst, cap, C.byref(n), C.byref(crc), C.byref(adler))
            assert rc == 0 and crc.value == zlib.crc32(data) and adler.value == zlib.adler32(data)
            _ref[key] = dst.raw[:n.value]
    return _ref[key]


def header(fmt, level=-1):
    return bytes([0x78, FLG[level]]) if fmt == ZLIB else GZ_HEADER if fmt == GZIP else b""


def trailer(fmt, whole):
    return (struct.pack(">I", zlib.adler32(whole)) if fmt == ZLIB else
            struct.pack("<II", zlib.crc32(whole), len(whole) & 0xffffffff) if fmt == GZIP else b"")


def carry_of(before, total_out=0, parts=0, status=0):
    return (zlib.crc32(before), zlib.adler32(before), len(before), total_out, parts, status)


def new_carry(eng, n, records=None):
    """n carry records on the device: `records` (tuples), or a pattern no call may leave behind"""
    c = np.zeros(max(n, 1), CY)
    c[:] = (0xdeadbeef, 0xfeedf00d, 1 << 40, 1 << 41, 77, 1)             # (finished, too: FIRST does not look)
    for i, r in enumerate(records or []):
        if r is not None:
            c[i] = r
    return eng.to_device(c)


class Part:
    """one job: data, the source bytes in front of it (prev), flags, and where prev lies: "contig" (just in front of src), an int (elsewhere,
    at that byte offset from a 16-byte boundary) or None (prev = NULL; prev_len = len(prev) all the same)"""

    def __init__(self, data, prev=b"", flags=0, place=3, cap_delta=0, src_off=0, dst_off=0, null_dst=False):
        self.data, self.prev, self.flags, self.place = data, prev[-PREV_KEEP:], flags, place
        self.cap_delta, self.src_off, self.dst_off, self.null_dst = cap_delta, src_off, dst_off, null_dst


class Call:
    """one call: every part's source (and prev) in one device buffer, the targets in slots of one device buffer filled with canary bytes.
    launch() queues it, collect() waits and reads everything back"""

    def __init__(self, eng, fc, fmt, hist_max, parts, carry, level=-1):
        import torch
        self.eng, self.fc, self.fmt, self.hist_max, self.level, self.parts, self.carry = eng, fc, fmt, hist_max, level, parts, carry
        n = len(parts)
        self.bound = [eng.deflate_stream_part_bound(len(p.data), hist_max, fmt, p.flags & 3) for p in parts]
        self.cap = [b + p.cap_delta for b, p in zip(self.bound, parts)]
        pos, sat, pat = 16, [], []
        for p in parts:
            a = (pos + 15) & ~15
            if p.place == "contig":
                s = (a + len(p.prev) + 15) & ~15
                pat.append(s - len(p.prev))
            elif p.place is None:
                s = a
                pat.append(None)
            else:
                pat.append(a + p.place)
                s = ((a + p.place + len(p.prev) + 15) & ~15) + 16          # a gap: prev + prev_len != src
            sat.append(s + p.src_off)
            pos = s + p.src_off + len(p.data) + 16
        hs = np.zeros(pos + 32, np.uint8)
        for p, s, a in zip(parts, sat, pat):
            if a is not None:
                hs[a:a + len(p.prev)] = np.frombuffer(p.prev, np.uint8)
            hs[s:s + len(p.data)] = np.frombuffer(p.data, np.uint8)
        self.dat, pos = [], 0
        for c, p in zip(self.cap, parts):
            self.dat.append(pos + 16 + p.dst_off)
            pos += (16 + p.dst_off + c + TAIL + 15) & ~15
        self.src = torch.from_numpy(hs).to(eng.dev)
        self.dst = torch.full((pos + 16,), CANARY, dtype=torch.uint8, device=eng.dev)
        self.j = np.zeros(n, PJ)
        for i, p in enumerate(parts):
            self.j[i] = (self.src.data_ptr() + sat[i], 0 if p.null_dst else self.dst.data_ptr() + self.dat[i], len(p.data), self.cap[i],
                         0 if pat[i] is None else self.src.data_ptr() + pat[i], len(p.prev), p.flags)
        self.slot_end = [a + c + TAIL for a, c in zip(self.dat, self.cap)]
        self.srcs = self.j["src"].copy()

    def launch(self):
        self.rc, self.dres = self.eng.deflate_stream_parts(self.fc, self.fmt, self.j, self.carry, hist_max=self.hist_max, level=self.level)
        self.j[:] = 0                                          # (the array may be reused as soon as the call returns)
        return self

    def collect(self):
        n = len(self.parts)
        self.res = self.eng.results_to_host(self.dres, SR)[:n].copy()
        self.cy = self.eng.results_to_host(self.carry, CY)[:n].copy()
        self.out = self.dst.cpu().numpy()
        return self

    def bytes(self, i):
        return self.out[self.dat[i]:self.dat[i] + int(self.res["out_len"][i])].tobytes()

    def untouched(self, i, used):
        """everything of slot i but its first `used` bytes still holds the canary"""
        lo = self.slot_end[i - 1] if i else 0
        return bool((self.out[lo:self.dat[i]] == CANARY).all() and (self.out[self.dat[i] + used:self.slot_end[i]] == CANARY).all())


def run(eng, fc, fmt, hist_max, parts, carry, level=-1):
    return Call(eng, fc, fmt, hist_max, parts, carry, level).launch().collect()


def expect(eng, fc, fmt, hist_max, p, before, level=-1):
    """the bytes part p must write when `before` is all of the stream's source in front of it"""
    return ((header(fmt, level) if p.flags & FIRST else b"") + host_part(eng, fc, p.data, p.flags & LAST, hist_max, before if p.prev else b"")
            + (trailer(fmt, before + p.data) if p.flags & LAST else b""))


def cut(lens, seed):
    """a source of sum(lens) mixed bytes cut into parts of these lengths"""
    whole, parts, at = mixed(sum(lens), seed), [], 0
    for n in lens:
        parts.append(whole[at:at + n])
        at += n
    return parts


def part_lens(B):
    """three streams whose parts take every length of {0, 1, 15, 16, B - 1, B, B + 1, 2 B + 17}, empty parts first, in the middle and last"""
    return [[B + 1, 0, 15, 2 * B + 17, 1, 16], [0, B, B - 1, 16, 0], [1, B - 1, 16, B + 1]]


def write_streams(eng, fc, fmt, hist_max, streams, level=-1, places=("contig", 0, 1, 7, 15), sync=True):
    """streams (lists of parts' bytes) written call by call, part k of every stream that has one in call k.  Returns per stream the list
    of (bytes written, result, carry) per part -- with sync=False the calls are queued back to back and read at the end"""
    n, depth = len(streams), max(len(s) for s in streams)
    calls = []
    carry = new_carry(eng, n)
    for k in range(depth):
        who = [i for i in range(n) if k < len(streams[i])]
        # a stream keeps its carry record: call k works on the records of the streams it holds, gathered in front
        sub = carry if len(who) == n else None
        parts = []
        for i in who:
            before = b"".join(streams[i][:k])
            flags = (FIRST if k == 0 else 0) | (LAST if k == len(streams[i]) - 1 else 0)
            parts.append(Part(streams[i][k], before, flags, places[(i + k) % len(places)]))
        if sub is None:
            import torch
            idx = torch.tensor(who, device=eng.dev)
            sub = carry.view(-1, CY.itemsize)[idx].contiguous().view(-1)
        c = Call(eng, fc, fmt, hist_max, parts, sub, level).launch()
        assert c.rc == 0
        if sync:
            c.collect()
        if sub is not carry:
            carry.view(-1, CY.itemsize)[idx] = sub.view(-1, CY.itemsize)
        calls.append((who, c))
    got = [[] for _ in range(n)]
    for who, c in calls:
        if not sync:
            c.collect()
        for slot, i in enumerate(who):
            assert c.untouched(slot, int(c.res["out_len"][slot])) or c.res["cc"][slot], (i, slot)
            got[i].append((c.bytes(slot), c.res[slot], c.cy[slot]))
    return got


@pytest.mark.parametrize("fmt", [RAW, ZLIB, GZIP])
@pytest.mark.parametrize("hist_max", [0, 4096, 32768])
@pytest.mark.parametrize("fc", [FHT, DHTGEN])
def test_every_part_is_the_host_paths_and_the_stream_inflates(eng, fc, hist_max, fmt):
    B, level = block_bytes(hist_max), 5
    streams = [cut(lens, 3 + i) for i, lens in enumerate(part_lens(B))]
    got = write_streams(eng, fc, fmt, hist_max, streams, level)
    for i, parts in enumerate(streams):
        whole, stream, total_out = b"".join(parts), b"", 0
        for k, data in enumerate(parts):
            s, r, cy = got[i][k]
            before = b"".join(parts[:k])
            flags = (FIRST if k == 0 else 0) | (LAST if k == len(parts) - 1 else 0)
            assert r["cc"] == 0, (i, k, r)
            want = ((header(fmt, level) if k == 0 else b"") + host_part(eng, fc, data, flags & LAST, hist_max, before)
                    + (trailer(fmt, whole) if flags & LAST else b""))
            assert s == want, "part %d of stream %d is not nxz_deflate_host_hist's (%d against %d bytes)" % (k, i, len(s), len(want))
            total_out += len(s)
            sofar = before + data
            assert tuple(int(x) for x in cy) == carry_of(sofar, total_out, k + 1, 1 if flags & LAST else 0), (i, k, cy)
            assert r["crc"] == zlib.crc32(sofar) and r["adler"] == zlib.adler32(sofar), (i, k, r)
            assert r["blocks"] == (len(data) + B - 1) // B and r["out_len"] == len(s), (i, k, r)
            stream += s
            if not flags & LAST:
                # a part ends on a byte boundary: what is written so far already yields every source byte so far
                assert zlib.decompressobj(WBITS[fmt]).decompress(stream) == sofar, (i, k)
        z = zlib.decompressobj(WBITS[fmt])
        assert z.decompress(stream) == whole and z.eof and z.unused_data == b"", i


@pytest.mark.parametrize("fmt", [ZLIB, GZIP])
def test_back_through_the_device_decoder(eng, fmt):
    import torch
    hist_max = 4096
    streams = [cut(lens, 11 + i) for i, lens in enumerate(part_lens(block_bytes(hist_max)))]
    got = write_streams(eng, DHTGEN, fmt, hist_max, streams)
    packed = [b"".join(s for s, _, _ in g) for g in got]
    n = len(packed)
    sat = np.concatenate([[0], np.cumsum([(len(p) + 31) & ~15 for p in packed])])
    dat = np.concatenate([[0], np.cumsum([(sum(map(len, s)) + 31) & ~15 for s in streams])])
    hs = np.zeros(int(sat[-1]) + 16, np.uint8)
    for p, a in zip(packed, sat):
        hs[a:a + len(p)] = np.frombuffer(p, np.uint8)
    src = torch.from_numpy(hs).to(eng.dev)
    back = torch.zeros(int(dat[-1]) + 16, dtype=torch.uint8, device=eng.dev)
    jobs = np.zeros(n, pkg.JOB_DTYPE)
    jobs["src"] = np.uint64(src.data_ptr()) + sat[:-1].astype(np.uint64)
    jobs["src_len"] = [len(p) for p in packed]
    jobs["dst"] = np.uint64(back.data_ptr()) + dat[:-1].astype(np.uint64)
    jobs["dst_cap"] = [sum(map(len, s)) for s in streams]
    jobs["in_adler"] = 1
    res, frames = eng.decompress_framed(fmt, eng.to_device(jobs), n)
    f, r = eng.frames_to_host(frames), eng.results_to_host(res)
    assert (f["status"][:n] == pkg.FRAME_OK).all() and (r["cc"][:n] == 0).all(), (f, r)
    bk = back.cpu().numpy()
    for i, s in enumerate(streams):
        whole = b"".join(s)
        assert r["tpbc"][i] == len(whole) and bk[dat[i]:dat[i] + len(whole)].tobytes() == whole, i


@pytest.mark.parametrize("fmt", [RAW, ZLIB, GZIP])
@pytest.mark.parametrize("hist_max", [0, 4096, 32768])
def test_first_and_last_is_the_plain_call(eng, hist_max, fmt):
    import torch
    bufs = edge_buffers(hist_max)
    for fc in (FHT, DHTGEN):
        c = run(eng, fc, fmt, hist_max, [Part(b, b"", FIRST | LAST) for b in bufs], new_carry(eng, len(bufs)), level=9)
        assert c.rc == 0 and (c.res["cc"] == 0).all()
        assert c.bound == [eng.deflate_stream_bound(len(b), hist_max, fmt) for b in bufs]
        # the plain call on the same sources and into a target of the same layout
        dst = torch.full_like(c.dst, CANARY)
        j = np.zeros(len(bufs), SJ)
        j["src"], j["src_len"], j["dst_cap"] = c.srcs, [len(b) for b in bufs], c.cap
        j["dst"] = np.uint64(dst.data_ptr()) + np.array(c.dat, np.uint64)
        rc, res = eng.deflate_stream_jobs(fc, fmt, j, hist_max=hist_max, level=9)
        assert rc == 0
        assert eng.results_to_host(res, SR)[:len(bufs)].tobytes() == c.res.tobytes(), fc
        assert np.array_equal(dst.cpu().numpy(), c.out), fc
        for i, b in enumerate(bufs):
            assert tuple(int(x) for x in c.cy[i]) == carry_of(b, int(c.res["out_len"][i]), 1, 1), i


@pytest.mark.parametrize("hist_max", [4096, 32768])
@pytest.mark.parametrize("fc", [FHT, DHTGEN])
def test_the_window_is_the_same_wherever_prev_lies(eng, fc, hist_max):
    H, B = hist_max, block_bytes(hist_max)
    before = mixed(3 * 32768, 22)                                       # (its last 32 KiB: random bytes)
    datas = [before[-3000:-1000] + jsonish(500, 2) + mixed(B + 17, 22), before[-700:] + jsonish(300, 3)]   # both repeat bytes of `before`
    prev_lens = [1, 15, 16, 4095, H, H + 5]
    places = ["contig", 0, 1, 7, 15]
    parts, what = [], []
    for di, data in enumerate(datas):
        for pl in prev_lens:
            for place in places:
                parts.append(Part(data, before[-pl:], 0, place))
                what.append((di, pl, place))
            if min(H, pl) & ~15 == 0:
                parts.append(Part(data, b"", 0, None))
                what.append((di, pl, None))
    c = run(eng, fc, ZLIB, hist_max, parts, new_carry(eng, len(parts), [carry_of(before)] * len(parts)))
    assert c.rc == 0 and (c.res["cc"] == 0).all(), c.res["cc"]
    seen = {}
    for slot, (di, pl, place) in enumerate(what):
        s = c.bytes(slot)
        assert c.untouched(slot, len(s)), what[slot]
        assert seen.setdefault((di, pl), s) == s, "prev at %r gives other bytes than prev at %r" % (place, places[0])
        assert tuple(int(x) for x in c.cy[slot]) == carry_of(before + datas[di], len(s), 1, 0), what[slot]
    for (di, pl), s in seen.items():
        assert s == host_part(eng, fc, datas[di], 0, hist_max, before[-pl:]), (di, pl)
    # the window is used: 2000 and 700 bytes of `before` come back as matches once the window reaches them
    assert len(seen[(1, H)]) < len(seen[(1, 16)]) - 300
    assert zlib.decompressobj(-15, zdict=before[-H:]).decompress(seen[(0, H)]) == datas[0]


def test_chunks_do_not_show(eng, monkeypatch):
    hist_max = 32768
    B = block_bytes(hist_max)
    before = mixed(40000, 31)
    # 18 blocks; first blocks that are staged at the batch's blocks 0, 1, 5, 7 and 11 to 14, contiguous ones at 4 and 15: chunks of 1, 2
    # and 3 hold none, one, two or three staged blocks, and streams straddle chunks
    datas = [jsonish(500, 1), mixed(3 * B - 1, 2), before[-900:] + make_block("alice", 1000, 3), b"", jsonish(B + 1, 4), mixed(3 * B + 5, 5),
             jsonish(700, 6), jsonish(717, 7), jsonish(734, 8), before[-5000:], mixed(2 * B + 17, 9)]
    places = [0, 7, "contig", 1, 15, 1, 0, 1, 7, 15, "contig"]
    flags = [0, LAST, 0, 0, LAST, 0, 0, LAST, 0, 0, LAST]

    def go():
        parts = [Part(d, before, f, p) for d, f, p in zip(datas, flags, places)]
        return run(eng, DHTGEN, GZIP, hist_max, parts, new_carry(eng, len(parts), [carry_of(before, 123, 4)] * len(parts)))

    monkeypatch.delenv("NXZ_STREAMS_CHUNK", raising=False)
    base = go()
    assert base.rc == 0 and (base.res["cc"] == 0).all() and list(base.res["blocks"][:6]) == [1, 3, 1, 0, 2, 4]
    for i, d in enumerate(datas):
        assert base.bytes(i) == expect(eng, DHTGEN, GZIP, hist_max, base.parts[i], before), i
        assert tuple(int(x) for x in base.cy[i]) == carry_of(before + d, 123 + int(base.res["out_len"][i]), 5, 1 if flags[i] else 0), i
    for chunk in (1, 2, 3):
        monkeypatch.setenv("NXZ_STREAMS_CHUNK", str(chunk))
        c = go()
        assert c.rc == 0
        assert c.res.tobytes() == base.res.tobytes() and c.cy.tobytes() == base.cy.tobytes(), chunk
        assert np.array_equal(c.out, base.out), chunk


def test_first_middle_last_and_whole_streams_in_one_call(eng):
    hist_max = 4096
    B = block_bytes(hist_max)
    before = [b"", mixed(70000, 41), mixed(B + 5, 42), b"", jsonish(20000, 43), mixed(100, 44)]
    datas = [mixed(B + 1, 45), jsonish(3000, 46), mixed(2 * B + 17, 47), jsonish(15, 48), b"", b""]
    flags = [FIRST, 0, LAST, FIRST | LAST, LAST, 0]
    places = [3, 1, "contig", 3, 7, 0]
    for fc, fmt in ((FHT, ZLIB), (DHTGEN, GZIP), (DHTGEN, RAW)):
        parts = [Part(d, b, f, p) for d, b, f, p in zip(datas, before, flags, places)]
        records = [None if f & FIRST else carry_of(b, 1000 + i, 2 + i) for i, (b, f) in enumerate(zip(before, flags))]
        c = run(eng, fc, fmt, hist_max, parts, new_carry(eng, len(parts), records))
        assert c.rc == 0 and (c.res["cc"] == 0).all(), c.res
        for i, p in enumerate(parts):
            s = c.bytes(i)
            assert s == expect(eng, fc, fmt, hist_max, p, before[i]) and c.untouched(i, len(s)), i
            was_out, was_parts = (0, 0) if flags[i] & FIRST else (1000 + i, 2 + i)
            assert tuple(int(x) for x in c.cy[i]) == carry_of(before[i] + datas[i], was_out + len(s), was_parts + 1, 1 if flags[i] & LAST else 0), i
            assert c.res["blocks"][i] == (len(datas[i]) + B - 1) // B, i
        assert c.bytes(5) == b"" and c.bytes(4) == bytes.fromhex("010000ffff") + trailer(fmt, before[4])
    # no part at all
    assert eng.deflate_stream_parts(DHTGEN, ZLIB, np.zeros(0, PJ), None)[0] == 0
    assert eng.deflate_stream_parts(DHTGEN, ZLIB, np.zeros(0, PJ), new_carry(eng, 0))[0] == 0


def test_refusals_among_good_parts(eng):
    hist_max, fmt = 32768, ZLIB
    before = mixed(50000, 51)
    good = lambda seed, flags=0: Part(mixed(70000, seed), before, flags, 1)      # noqa: E731
    data = jsonish(5000, 52)
    parts = [good(53), Part(data, before[-500:], 0, None),                       # 1: prev NULL with prev_len != 0
             Part(data, before, 4, 1), good(54, LAST),                           # 2: a flag bit that is none
             Part(data, before[-16:], FIRST, 1),                                 # 4: FIRST with prev_len != 0
             Part(data, before, 0, 1), good(55),                                 # 5: no FIRST on a finished carry
             Part(data, before, LAST, 1, cap_delta=-1),                          # 7: a byte too few
             Part(data, before, 0, 1, src_off=8),                                # 8: the plain call's: src not aligned
             Part(data, before, 0, 1, null_dst=True), Part(data, b"", FIRST | LAST | 8, 3), good(56)]
    refused = {1: INVALID_OP, 2: INVALID_OP, 4: INVALID_OP, 5: INVALID_OP, 7: TARGET_SPACE, 8: INVALID_OP, 9: INVALID_OP, 10: INVALID_OP}
    records = [carry_of(before, 900 + i, 3, 1 if i == 5 else 0) for i in range(len(parts))]
    c = run(eng, DHTGEN, fmt, hist_max, parts, new_carry(eng, len(parts), records))
    assert c.rc == 0
    assert list(c.res["cc"]) == [refused.get(i, 0) for i in range(len(parts))]
    for i, p in enumerate(parts):
        if i in refused:
            assert c.untouched(i, 0), i                                          # canaries in front, behind and all through the slot
            assert tuple(int(x) for x in c.cy[i]) == records[i], i
            assert c.res["out_len"][i] == (c.bound[i] if refused[i] == TARGET_SPACE else 0) and c.res["blocks"][i] == 0, i
            assert c.res["crc"][i] == 0 and c.res["adler"][i] == 0 and c.res["stored"][i] == 0, i
        else:
            s = c.bytes(i)
            assert s == expect(eng, DHTGEN, fmt, hist_max, p, before) and c.untouched(i, len(s)), i
            assert tuple(int(x) for x in c.cy[i]) == carry_of(before + p.data, 900 + i + len(s), 4, 1 if p.flags & LAST else 0), i
    assert c.bound[7] == eng.deflate_stream_bound(5000, hist_max, RAW) + 4
    # the refused part again, with room and on the carry it left alone
    again = run(eng, DHTGEN, fmt, hist_max, [Part(data, before, LAST, 1)], new_carry(eng, 1, [records[7]]))
    assert again.rc == 0 and again.res["cc"][0] == 0
    assert again.bytes(0) == expect(eng, DHTGEN, fmt, hist_max, again.parts[0], before)
    assert tuple(int(x) for x in again.cy[0]) == carry_of(before + data, 907 + len(again.bytes(0)), 4, 1)
    # what the call does not take at all
    j, cy = np.zeros(1, PJ), new_carry(eng, 1)
    assert eng.deflate_stream_parts(DHTGEN, fmt, j, None)[0] == -errno.EINVAL
    assert eng.deflate_stream_parts(pkg.FC_COMPRESS_DHT, fmt, j, cy)[0] == -errno.EINVAL
    assert eng.deflate_stream_parts(DHTGEN, 3, j, cy)[0] == -errno.EINVAL
    assert eng.deflate_stream_parts(DHTGEN, fmt, j, cy, level=10)[0] == -errno.EINVAL
    assert eng.L.nxz_batch_deflate_streams_part(eng.ctx, DHTGEN, fmt, -1, 0, None, 1, cy.data_ptr(), cy.data_ptr(), None) == -errno.EINVAL
    assert eng.L.nxz_batch_deflate_streams_part(eng.ctx, DHTGEN, fmt, -1, 0, j.ctypes.data, 1, cy.data_ptr(), None, None) == -errno.EINVAL


@pytest.mark.parametrize("fc,fmt,hist_max", [(DHTGEN, GZIP, 32768), (FHT, ZLIB, 4096), (DHTGEN, RAW, 0)])
def test_calls_chain_on_the_device(eng, fc, fmt, hist_max):
    B = block_bytes(hist_max)
    streams = [cut([B + 1, 2 * B + 17, 15], 61), cut([16, 0, B], 62), cut([B - 1, 1, B + 1], 63)]
    waited = write_streams(eng, fc, fmt, hist_max, streams)
    queued = write_streams(eng, fc, fmt, hist_max, streams, sync=False)          # three calls back to back, one wait at the end
    for i, (w, q) in enumerate(zip(waited, queued)):
        assert [s for s, _, _ in w] == [s for s, _, _ in q], i
        assert all(rw.tobytes() == rq.tobytes() for (_, rw, _), (_, rq, _) in zip(w, q)), i
        # the record is one: with no wait in between it is read once, at the end -- the stream's last carry
        assert q[-1][2].tobytes() == w[-1][2].tobytes() and q[-1][2]["status"] == 1, i
        whole = b"".join(streams[i])
        assert zlib.decompressobj(WBITS[fmt]).decompress(b"".join(s for s, _, _ in q)) == whole, i
