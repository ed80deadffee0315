"""GPU tests of the compress side's output edges (include/nxz_engine.h).

Part A: every emitter of nxz_batch_compress / nxz_batch_compress_dict and nxz_batch_wrap with dst_cap around the exact output
length, in canary-filled slots of one device tensor: the oracle's bytes and results when the target fits, cc 13 / tpbc 0 when it
does not, and in both cases not a byte outside [dst, dst + what the job may write).  The cases and what they cover are
tests/compress_edge_cases.py's (checked on the CPU by tests/test_compress_edge_cases_host.py).

Part B: nxz_batch_pack_gzip / _zlib / _zlib_dict on hand-made jobs and results (tests/pack_cases.py) against the byte-exact model
tests/pack_model.py, `packed` held to the byte between two guards."""
import gzip
import importlib
import os
import zlib

import numpy as np
import pytest

import compress_edge_cases as E
import pack_cases as PC
import pack_model as M
from datagen import make_block

pytestmark = pytest.mark.gpu
pkg = importlib.import_module("power-gzip_amd")

CANARY = 0xA5
GUARD = 64
KNOBS = ("NXZ_FUSED_GEN",)


@pytest.fixture(scope="module")
def eng():
    saved = {k: os.environ.pop(k, None) for k in KNOBS}
    e = pkg.Engine(0)
    yield e
    e.close()
    for k, v in saved.items():
        if v is not None:
            os.environ[k] = v


def up16(n):
    return (n + 15) & ~15


# ---- part B: the member packers against the model -----------------------------------------------------------------------------
class Launch:
    """the cases of one launch on the device: sources and outputs in 16-byte aligned slots, jobs[] and results[] made by hand"""

    def __init__(self, eng, cases):
        import torch
        self.cases, self.n = cases, len(cases)
        soff = np.cumsum([0] + [up16(len(c[6])) + 16 for c in cases])
        doff = np.cumsum([0] + [up16(len(c[7])) + 16 for c in cases])
        self.src_host = np.full(int(soff[-1]), 0x11, np.uint8)
        self.dst_host = np.full(int(doff[-1]), 0x22, np.uint8)
        for i, c in enumerate(cases):
            self.src_host[soff[i]:soff[i] + len(c[6])] = np.frombuffer(c[6], np.uint8)
            self.dst_host[doff[i]:doff[i] + len(c[7])] = np.frombuffer(c[7], np.uint8)
        self.src = torch.from_numpy(self.src_host).to(eng.dev)
        self.dst = torch.from_numpy(self.dst_host).to(eng.dev)
        j = np.zeros(self.n, pkg.JOB_DTYPE)
        r = np.zeros(self.n, pkg.RESULT_DTYPE)
        j["src"] = np.uint64(self.src.data_ptr()) + soff[:-1].astype(np.uint64)
        j["dst"] = np.uint64(self.dst.data_ptr()) + doff[:-1].astype(np.uint64)
        j["src_len"] = [c[0] + c[1] for c in cases]
        j["hist_len"] = [c[1] for c in cases]
        j["dst_cap"] = [PC.compress_bound(c[0]) for c in cases]
        j["in_adler"] = 1
        r["cc"] = [c[2] for c in cases]
        r["tpbc"] = [c[3] for c in cases]
        r["spbc"] = j["src_len"]
        r["crc"] = [c[4] for c in cases]
        r["adler"] = [c[5] for c in cases]
        self.jobs, self.results = eng.to_device(j), eng.to_device(r)


@pytest.fixture(scope="module")
def launches(eng):
    return {name: Launch(eng, cases) for name, cases in PC.launches().items()}


@pytest.fixture(scope="module")
def pack_dict(eng):
    d = eng.dict_create(PC.DICT)
    yield d
    d.close()


def run_packer(eng, packer, level, d, jobs, results, n, packed):
    if packer == "gzip":
        return eng.pack_gzip(jobs, results, n, packed)
    if packer == "zlib":
        return eng.pack_zlib(level, jobs, results, n, packed)
    return eng.pack_zlib_dict(level, d, jobs, results, n, packed)


def check_pack(eng, packer, level, d, jobs, results, cases, shift, what):
    """one launch into a buffer of exactly the model's total at `shift` bytes past a 16-byte boundary, guards on both sides"""
    import torch
    n = len(cases)
    want_off, want = M.image(packer, cases, level=level, dictid=d.id if d is not None else 0)
    total = want_off[-1]
    front = GUARD + shift
    buf = torch.full((front + total + GUARD + 4096,), CANARY, dtype=torch.uint8, device=eng.dev)
    offs = run_packer(eng, packer, level, d, jobs, results, n, buf[front:])
    torch.cuda.synchronize(eng.dev)
    got_off = [int(x) for x in offs.cpu().numpy()]
    got = buf.cpu().numpy()
    assert got_off[0] == 0 and len(got_off) == n + 1
    # member by member at the offsets the device gave, so that a wrong member is named and the ones behind it are still looked at
    bad = []
    for i, c in enumerate(cases):
        lo, hi = got_off[i], got_off[i + 1]
        if not (0 <= lo <= hi <= total) or got[front + lo:front + hi].tobytes() != want[want_off[i]:want_off[i + 1]]:
            bad.append((i, "length %d hist %d cc %d tpbc %d" % c[:4]))
    assert not bad, (what, bad[:12], len(bad))
    assert got_off == want_off, what
    assert got[front:front + total].tobytes() == want, what
    assert (got[:front] == CANARY).all() and (got[front + total:] == CANARY).all(), what


PACKERS = [("gzip", -1)] + [("zlib", lv) for lv in (-1, 0, 1, 5, 9)] + [("zlib_dict", -1), ("zlib_dict", 9)]


@pytest.mark.parametrize("packer,level", PACKERS, ids=["%s%+d" % p for p in PACKERS])
def test_packers_against_the_model(eng, launches, pack_dict, packer, level):
    """every launch of tests/pack_cases.py; the header puts no alignment on `packed`, so the table and the 1025 launch are also
    packed at +1, +2 and +3: every member then starts at every residue mod 4"""
    d = pack_dict if packer == "zlib_dict" else None
    assert d is None or d.id == zlib.adler32(PC.DICT)
    for name, la in launches.items():
        for shift in (0, 1, 2, 3) if name in ("table", "1025") else (0,):
            check_pack(eng, packer, level, d, la.jobs, la.results, la.cases, shift, (name, shift))
    for la in launches.values():                        # the packers read src and dst, nothing else
        assert (la.src.cpu().numpy() == la.src_host).all() and (la.dst.cpu().numpy() == la.dst_host).all()


def test_pack_blocks_of_65536_bytes(eng, pack_dict):
    """real blocks of the largest size a job may carry: one that does not shrink, two that do, each also with a target too small
    (cc 13).  The fallbacks are two stored blocks each; every member decodes; the images are the model's from the real results."""
    import torch
    blocks = [make_block(k, 65536, seed=3) for k in ("random", "alice", "zeros")] * 2
    caps = [73856] * 3 + [4096, 4096, 16]
    n = len(blocks)
    src = torch.from_numpy(np.frombuffer(b"".join(blocks), np.uint8).copy()).to(eng.dev)
    cdst = torch.zeros((n, 73856), dtype=torch.uint8, device=eng.dev)
    jobs = eng.jobs_strided(src, 65536, np.full(n, 65536, np.uint32), cdst, 73856, np.array(caps, np.uint32))
    res, _ = eng.compress(pkg.FC_COMPRESS_DHTGEN, jobs, n)
    r = eng.results_to_host(res)
    out = cdst.cpu().numpy()
    assert [int(x) for x in r["cc"]] == [64, 0, 0, 13, 13, 13] and r["tpbc"][0] >= 65536 + 5
    cases = [(65536, 0, int(r["cc"][i]), int(r["tpbc"][i]), int(r["crc"][i]), int(r["adler"][i]), blocks[i], out[i].tobytes())
             for i in range(n)]
    assert [M.is_stored(c[0], c[2], c[3]) for c in cases] == [True, False, False, True, True, True]
    # a job that failed for want of space still reports the source's checksums: its stored member needs them
    assert [int(x) for x in r["crc"]] == [zlib.crc32(b) for b in blocks] and [int(x) for x in r["adler"]] == [zlib.adler32(b) for b in blocks]
    for packer, level, d in (("gzip", -1, None), ("zlib", 5, None), ("zlib_dict", -1, pack_dict)):
        check_pack(eng, packer, level, d, jobs, res, cases, 0, packer)
        offs, img = M.image(packer, cases, level=level, dictid=pack_dict.id)
        for i, b in enumerate(blocks):
            m = img[offs[i]:offs[i + 1]]
            if packer == "gzip":
                assert gzip.decompress(m) == b, i
            elif packer == "zlib":
                assert zlib.decompress(m) == b, i
            else:
                dz = zlib.decompressobj(zdict=PC.DICT)
                assert dz.decompress(m) == b and dz.eof, i


# ---- part A: dst_cap around the exact length ------------------------------------------------------------------------------------
FRONT, BEHIND, TAIL = 16, 64, 32768      # canary in front of every dst and behind its dst_cap; behind the last slot, room for a
#                                          block written in full by an emitter that forgot dst_cap (the longest is 9 KiB)


def slots(eng, caps):
    """one canary-filled device tensor with a 16-byte aligned slot per job: [FRONT][dst_cap rounded up to 16][BEHIND]"""
    import torch
    sizes = [FRONT + up16(c) + BEHIND for c in caps]
    start = np.cumsum([0] + sizes)
    dst = torch.full((int(start[-1]) + TAIL,), CANARY, dtype=torch.uint8, device=eng.dev)
    assert dst.data_ptr() % 16 == 0
    return dst, [int(s) + FRONT for s in start[:-1]], [int(s) for s in start[1:]]


def sources(eng, blobs):
    import torch
    off = np.cumsum([0] + [up16(len(b)) + 16 for b in blobs])
    host = np.zeros(int(off[-1]), np.uint8)
    for o, b in zip(off, blobs):
        host[o:o + len(b)] = np.frombuffer(b, np.uint8)
    return torch.from_numpy(host).to(eng.dev), [int(o) for o in off[:-1]]


@pytest.mark.parametrize("emitter", list(E.EMITTERS))
def test_compress_target_around_the_exact_length(eng, emitter):
    """every (block, dst_cap) of the emitter's class as one job of one launch.  A target that fits: the oracle's bytes and results,
    nothing behind tpbc.  One that does not: cc 13, tpbc 0, nothing at or behind dst + dst_cap (what stands below is not looked
    at).  Never a byte in front of dst.  The COUNT codes count before anything is written: the 316 counts are the oracle's for
    every job, short target or not (include/nxz_engine.h makes no exception for a failed job)."""
    form, cls, env, through_dict = E.EMITTERS[emitter]
    fc = getattr(pkg, "FC_COMPRESS_" + form)
    cs = E.cases(cls)
    src, soff = sources(eng, [c.body if through_dict else c.data for c in cs])
    jobs_in = [(ci, cap) for ci, c in enumerate(cs) for cap in c.caps()]
    n = len(jobs_in)
    dst, doff, dend = slots(eng, [cap for _, cap in jobs_in])
    j = np.zeros(n, pkg.JOB_DTYPE)
    j["src"] = [src.data_ptr() + soff[ci] for ci, _ in jobs_in]
    j["dst"] = [dst.data_ptr() + o for o in doff]
    j["src_len"] = [len(cs[ci].body) if through_dict else len(cs[ci].data) for ci, _ in jobs_in]
    j["hist_len"] = [0 if through_dict else len(cs[ci].hist) for ci, _ in jobs_in]
    j["dst_cap"] = [cap for _, cap in jobs_in]
    j["in_adler"] = 1
    jobs = eng.to_device(j)
    dht, d = None, None
    if form == "DHT":
        arr = np.zeros(1, pkg.DHT_DTYPE)
        bits, nb = E.canned_table()
        arr["dhtlen"][0] = nb
        arr["dht"][0, :len(bits)] = np.frombuffer(bits, np.uint8)
        dht = eng.to_device(arr)
    os.environ.update(env)
    try:
        if through_dict:
            d = eng.dict_create(E.DICT)
            assert d.deflate_window == len(E.dict_window())
            res, cnt = eng.compress_dict(fc, d, jobs, n)
        else:
            res, cnt = eng.compress(fc, jobs, n, dht=dht, ntables=1 if dht is not None else 0)
        r = eng.results_to_host(res)
    finally:
        for k in env:
            os.environ.pop(k, None)
        if d is not None:
            d.close()
    out = dst.cpu().numpy()
    cnt = cnt.cpu().numpy().view(np.uint32).reshape(n, 316) if cnt is not None else None
    assert (fc & 4 != 0) == (cnt is not None)
    bad = []
    for i, (ci, cap) in enumerate(jobs_in):
        c, o = cs[ci], doff[i]
        got = tuple(int(r[k][i]) for k in ("cc", "tpbc", "tebc", "spbc", "crc", "adler"))
        why = []
        if not (out[o - FRONT:o] == CANARY).all():
            why.append("written in front of dst")
        if cap >= c.L:
            want = (c.cc, c.L, c.tebc, len(c.body) if through_dict else len(c.data), zlib.crc32(c.body), zlib.adler32(c.body))
            if got != want:
                why.append("results %r, not %r" % (got, want))
            if out[o:o + c.L].tobytes() != c.exp:
                why.append("bytes differ")
            if not (out[o + c.L:dend[i]] == CANARY).all():
                why.append("written behind tpbc")
        else:
            if got[:2] != (13, 0):
                why.append("cc %d tpbc %d, not 13 and 0" % got[:2])
            if not (out[o + cap:dend[i]] == CANARY).all():
                why.append("written at or behind dst + dst_cap")
        if cnt is not None and not (cnt[i] == c.counts).all():
            why.append("counts differ")
        if why:
            bad.append((c.name, "L %d" % c.L, "cap %d" % cap, why))
    assert not bad, (len(bad), bad[:10])
    assert (out[dend[-1]:] == CANARY).all()


def test_wrap_target_around_the_length(eng):
    """nxz_batch_wrap with dst_cap = n - 1, n, n + 1: short -- cc 13, tpbc 0, the slot untouched; fitting -- the bytes, the checksums,
    nothing behind them"""
    blocks = [make_block("random", n, seed=n + 1) for n in E.WRAP_SIZES]
    src, soff = sources(eng, blocks)
    jobs_in = [(bi, cap) for bi, b in enumerate(blocks) for cap in (len(b) - 1, len(b), len(b) + 1) if cap >= 0]
    n = len(jobs_in)
    dst, doff, dend = slots(eng, [cap for _, cap in jobs_in])
    j = np.zeros(n, pkg.JOB_DTYPE)
    j["src"] = [src.data_ptr() + soff[bi] for bi, _ in jobs_in]
    j["dst"] = [dst.data_ptr() + o for o in doff]
    j["src_len"] = [len(blocks[bi]) for bi, _ in jobs_in]
    j["dst_cap"] = [cap for _, cap in jobs_in]
    j["in_adler"] = 1
    r = eng.results_to_host(eng.wrap(eng.to_device(j), n))
    out = dst.cpu().numpy()
    assert sum(cap < len(blocks[bi]) for bi, cap in jobs_in) == len(blocks) - 1
    for i, (bi, cap) in enumerate(jobs_in):
        b, o, where = blocks[bi], doff[i], (len(blocks[bi]), cap)
        if cap < len(b):
            assert r["cc"][i] == 13 and r["tpbc"][i] == 0, where
            assert (out[o - FRONT:dend[i]] == CANARY).all(), where
        else:
            assert r["cc"][i] == 0 and r["tpbc"][i] == len(b) and r["spbc"][i] == len(b), where
            assert r["crc"][i] == zlib.crc32(b) and r["adler"][i] == zlib.adler32(b), where
            assert out[o:o + len(b)].tobytes() == b, where
            assert (out[o - FRONT:o] == CANARY).all() and (out[o + len(b):dend[i]] == CANARY).all(), where
    assert (out[dend[-1]:] == CANARY).all()
