"""GPU tests of nxz_batch_shuffle / nxz_batch_unshuffle (include/nxz_engine.h; the kernel in power-gzip_amd/csrc/nxz_shuffle.hip, the rules in
nxz_shuffle.h).  Every output is compared byte for byte with tests/shuffle_model.py.  Sources and targets of a batch lie in ONE device
arena that is canary everywhere else -- 64 bytes in front of and behind every buffer at the least -- and the whole arena is compared
with what it must hold afterwards: a byte written outside a target, or a source that changed, shows wherever it lies."""
import errno
import importlib
import zlib

import numpy as np
import pytest

from shuffle_model import shuffle, unshuffle

pytestmark = pytest.mark.gpu
pkg = importlib.import_module("power-gzip_amd")
E = pkg.engine
SJ = E.SHUFFLE_JOB_DTYPE
CANARY, GUARD = 0xc3, 64
INVALID_OP = 8
ELEMS = [1, 2, 3, 4, 6, 8, 12, 16, 17, 255, 256]
OFFS = [0, 1, 7, 15]


@pytest.fixture(scope="module")
def eng():
    e = pkg.Engine(0)
    yield e
    e.close()


class Arena:
    """buffers at chosen offsets from a 16-byte boundary, canary between them; `want` is what the device must hold in the end"""

    def __init__(self):
        self.parts, self.size = [], 0

    def add(self, off, data=None, size=None):
        """a buffer `off` bytes behind a 16-byte boundary, holding `data` (or `size` bytes of canary: a target) -> its position"""
        size = len(data) if data is not None else size
        pos = ((self.size + GUARD + 15) & ~15) + off
        if data is not None:
            self.parts.append((pos, np.frombuffer(bytes(data), np.uint8)))
        self.size = pos + size + GUARD
        return pos

    def upload(self, eng):
        import torch
        self.host = np.full(self.size + 16, CANARY, np.uint8)
        for pos, d in self.parts:
            self.host[pos:pos + len(d)] = d
        self.want = self.host.copy()
        self.dev = torch.from_numpy(self.host).to(eng.dev)
        assert self.dev.data_ptr() % 16 == 0
        return self.dev.data_ptr()

    def expect(self, pos, data):
        self.want[pos:pos + len(data)] = np.frombuffer(bytes(data), np.uint8)

    def check(self, what=""):
        got = self.dev.cpu().numpy()
        if not np.array_equal(got, self.want):
            at = int(np.flatnonzero(got != self.want)[0])
            raise AssertionError("%s: the arena differs first at byte %d (got %#x, want %#x)" % (what, at, got[at], self.want[at]))


def run(eng, cases, undo, what=""):
    """cases: (data, elem, src_off, dst_off).  One call; every target against the model, every other byte of the arena unchanged."""
    a = Arena()
    spos = [a.add(so, data=d) for d, _, so, _ in cases]
    dpos = [a.add(do, size=len(d)) for d, _, _, do in cases]
    base = a.upload(eng)
    j = np.zeros(len(cases), SJ)
    for i, (d, elem, _, _) in enumerate(cases):
        j[i] = (base + spos[i], base + dpos[i], len(d), elem, 0)
        a.expect(dpos[i], (unshuffle if undo else shuffle)(d, elem))
    rc, status = eng.shuffle(j, undo=undo)
    assert rc == 0
    eng.torch.cuda.synchronize(eng.dev)
    st = status.cpu().numpy()[:len(cases)]
    assert (st == 0).all(), (what, np.flatnonzero(st != 0)[:10])
    a.check(what)


def edge_lens(eng, elem):
    T = eng.shuffle_tile_elems(elem)
    assert T > 0 and T % 16 == 0
    tile = T * elem
    lens = [0, 1, elem - 1, elem, elem + 1, 15, 16, 17, 16 * elem - 1, 16 * elem + 1, tile - elem, tile + elem, tile - 1, tile, tile + 1, 2 * tile + 5]
    return sorted(set(n for n in lens if n >= 0))


@pytest.mark.parametrize("undo", [False, True], ids=["shuffle", "unshuffle"])
@pytest.mark.parametrize("elem", ELEMS)
def test_edge_grid(eng, elem, undo):
    rnd = np.random.default_rng(elem)
    cases = []
    for n in edge_lens(eng, elem):
        data = rnd.integers(0, 256, n, dtype=np.uint8).tobytes()
        for so in OFFS:
            for do in OFFS:
                cases.append((data, elem, so, do))
    run(eng, cases, undo, "elem %d" % elem)


def test_tile_query(eng):
    assert eng.shuffle_tile_elems(0) == 0 and eng.shuffle_tile_elems(257) == 0
    for elem in range(1, 257):
        T = eng.shuffle_tile_elems(elem)
        assert T % 16 == 0 and 64 <= T and T * elem <= 16384


@pytest.mark.parametrize("undo", [False, True], ids=["shuffle", "unshuffle"])
def test_ragged_batch_twice_without_a_wait(eng, undo):
    rnd = np.random.default_rng(7)
    big = 3 * (1 << 20) + 5
    cases = []
    for i in range(3000):
        elem = int(rnd.choice([1, 2, 3, 4, 5, 7, 8, 12, 16, 17, 31, 100, 255, 256]))
        cases.append((rnd.integers(0, 256, int(rnd.integers(0, 601)), dtype=np.uint8).tobytes(), elem, int(rnd.integers(0, 16)), int(rnd.integers(0, 16))))
    for k, elem in zip((200, 1500, 2800), (4, 2, 6)):
        cases.insert(k, (rnd.integers(0, 256, big, dtype=np.uint8).tobytes(), elem, 1, 7))
    a = Arena()
    spos = [a.add(so, data=d) for d, _, so, _ in cases]
    dpos = [[a.add(do, size=len(d)) for d, _, _, do in cases] for _ in range(2)]
    base = a.upload(eng)
    j = np.zeros(len(cases), SJ)
    for i, (d, elem, _, _) in enumerate(cases):
        j[i] = (base + spos[i], base + dpos[0][i], len(d), elem, 0)
        out = (unshuffle if undo else shuffle)(d, elem)
        a.expect(dpos[0][i], out)
        a.expect(dpos[1][i], out)
    rc, st0 = eng.shuffle(j, undo=undo)
    assert rc == 0
    # the same jobs again, behind the first call on the same stream and with no wait: the host array is the caller's again
    j["dst"] = [base + p for p in dpos[1]]
    rc, st1 = eng.shuffle(j, undo=undo)
    assert rc == 0
    eng.torch.cuda.synchronize(eng.dev)
    assert (st0.cpu().numpy() == 0).all() and (st1.cpu().numpy() == 0).all()
    a.check("ragged")


@pytest.mark.parametrize("undo", [False, True], ids=["shuffle", "unshuffle"])
def test_refusals_among_good_jobs(eng, undo):
    t = eng.torch
    rnd = np.random.default_rng(11)
    n = 1000
    data = rnd.integers(0, 256, n, dtype=np.uint8).tobytes()
    a = Arena()
    s = a.add(1, data=data)
    # good, src NULL, good, dst NULL, good, elem 0, good, elem 257, good, reserved, good, src == dst, good, overlap by a byte either way, good,
    # then ranges that touch (taken), an empty job with NULLs and an empty job with src == dst (taken)
    d = [a.add(7, size=n) for _ in range(18)]
    two = a.add(3, data=data + bytes([CANARY]) * n)                      # a source with its target right behind it
    base = a.upload(eng)
    B = lambda p: base + p
    jobs = [(B(s), B(d[0]), n, 4, 0), (0, B(d[1]), n, 4, 0), (B(s), B(d[2]), n, 3, 0), (B(s), 0, n, 4, 0), (B(s), B(d[4]), n, 8, 0),
            (B(s), B(d[5]), n, 0, 0), (B(s), B(d[6]), n, 16, 0), (B(s), B(d[7]), n, 257, 0), (B(s), B(d[8]), n, 17, 0),
            (B(s), B(d[9]), n, 4, 1), (B(s), B(d[10]), n, 2, 0), (B(d[11]), B(d[11]), n, 4, 0), (B(s), B(d[12]), n, 256, 0),
            (B(d[13]), B(d[13]) + n - 1, n, 4, 0), (B(d[14]) + n - 1, B(d[14]), n, 4, 0), (B(s), B(d[15]), n, 1, 0),
            (B(two), B(two) + n, n, 4, 0), (0, 0, 0, 4, 0), (B(d[16]), B(d[16]), 0, 4, 0), (B(s), B(d[17]), n, 6, 0)]
    want = [0, INVALID_OP, 0, INVALID_OP, 0, INVALID_OP, 0, INVALID_OP, 0, INVALID_OP, 0, INVALID_OP, 0, INVALID_OP, INVALID_OP, 0, 0, 0, 0, 0]
    j = np.zeros(len(jobs), SJ)
    for i, job in enumerate(jobs):
        j[i] = job
        if want[i] == 0 and job[2]:
            a.expect(job[1] - base, (unshuffle if undo else shuffle)(data, job[3]))
    status = t.full((len(jobs),), 77, dtype=t.int32, device=eng.dev)
    rc, status = eng.shuffle(j, status=status, undo=undo)
    assert rc == 0
    eng.torch.cuda.synchronize(eng.dev)
    assert status.cpu().numpy().tolist() == want
    a.check("refusals")                                                  # a refused job's target is all canary, its neighbours exact


def test_call_level_returns(eng):
    t = eng.torch
    assert eng.shuffle(np.zeros(0, SJ))[0] == 0 and eng.shuffle(np.zeros(0, SJ), undo=True)[0] == 0
    assert eng.shuffle(np.zeros(0, SJ), status=False)[0] == 0           # n == 0: nothing is looked at
    buf = t.zeros(64, dtype=t.uint8, device=eng.dev)
    j = np.zeros(1, SJ)
    j[0] = (buf.data_ptr(), buf.data_ptr() + 32, 16, 4, 0)
    for undo in (False, True):
        assert eng.shuffle(j, status=False, undo=undo)[0] == -errno.EINVAL
    f = eng.L.nxz_batch_shuffle
    st = t.zeros(1, dtype=t.int32, device=eng.dev)
    assert f(None, j.ctypes.data, 1, st.data_ptr(), eng.stream_handle()) == -errno.EINVAL
    assert f(eng.ctx, None, 1, st.data_ptr(), eng.stream_handle()) == -errno.EINVAL
    assert f(eng.ctx, j.ctypes.data, 1 << 31, st.data_ptr(), eng.stream_handle()) == -errno.E2BIG
    eng.torch.cuda.synchronize(eng.dev)
    assert not buf.cpu().numpy().any()


def numeric_buffers():
    rnd = np.random.default_rng(26)
    walk = np.cumsum(rnd.normal(0, 1, 1 << 18)).astype(np.float32)                      # 1 MiB
    w32 = rnd.normal(0, 0.02, 1 << 16).astype(np.float32)                                # 256 KiB
    bf16 = (rnd.normal(0, 0.02, 1 << 17).astype(np.float32).view(np.uint32) >> 16).astype(np.uint16)   # 256 KiB
    ids = (np.arange(1 << 13, dtype=np.int64) * 3 + rnd.integers(0, 3, 1 << 13)) + (1 << 40)           # 64 KiB
    return [(walk, 4), (w32, 4), (bf16, 2), (ids, 8)]


def test_round_trip_through_the_codec(eng):
    t = eng.torch
    for arr, elem in numeric_buffers():
        raw = arr.tobytes()
        assert arr.itemsize == elem and 65536 <= len(raw) <= 1 << 20
        src = eng.to_device(np.frombuffer(raw, np.uint8))
        sh, offs, st = eng.shuffle_bufs([src], elem)
        out, ooffs, res = eng.deflate_streams(pkg.FC_COMPRESS_DHTGEN, E.FMT_ZLIB, [sh[:len(raw)]])
        r = eng.results_to_host(res, E.STREAM_RESULT_DTYPE)
        assert st.cpu().numpy()[0] == 0 and r["cc"][0] == 0
        stream = out[:int(r["out_len"][0])].cpu().numpy().tobytes()
        # what an HDF5 or Zarr reader relies on: a zlib stream of the shuffled bytes
        assert zlib.decompress(stream) == shuffle(raw, elem)
        back = t.zeros(len(raw) + 16, dtype=t.uint8, device=eng.dev)
        j = np.zeros(1, pkg.JOB_DTYPE)
        j[0]["src"], j[0]["src_len"], j[0]["dst"], j[0]["dst_cap"], j[0]["in_adler"] = out.data_ptr(), len(stream), back.data_ptr(), len(raw), 1
        dres, frames = eng.decompress_framed(E.FMT_ZLIB, eng.to_device(j), 1)
        un, _, st2 = eng.shuffle_bufs([back[:len(raw)]], elem, undo=True)
        f, dr = eng.frames_to_host(frames), eng.results_to_host(dres)
        assert f["status"][0] == pkg.FRAME_OK and dr["cc"][0] == 0 and dr["tpbc"][0] == len(raw)
        assert st2.cpu().numpy()[0] == 0 and un[:len(raw)].cpu().numpy().tobytes() == raw, elem
        # (printed, not asserted: what the filter is worth on this buffer)
        plain = eng.results_to_host(eng.deflate_streams(pkg.FC_COMPRESS_DHTGEN, E.FMT_ZLIB, [src])[2], E.STREAM_RESULT_DTYPE)
        print("elem %d, %d bytes: plain %d, shuffled %d" % (elem, len(raw), plain["out_len"][0], len(stream)))
