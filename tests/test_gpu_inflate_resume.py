"""What every inflate route does with the resume state a job brings IN (in_sfbt, in_subc, in_rembytecnt, the table of an
open dynamic block, history, checksum seeds), against the CPU oracle: the cases of tests/resume_cases.py -- second halves
of streams cut inside headers, tables and block bodies, their first halves decoded by the oracle -- as one batch per
route, the same through nxu_run_job (FC 0x14) against the CPU engine model, and broken state between good jobs."""
import ctypes as C
import importlib
import zlib

import numpy as np
import pytest

import oracle_lib as O
import resume_cases as R
from inflate_routes import ROUTES, inflate_route
from run_job import run_both

pytestmark = pytest.mark.gpu
pkg = importlib.import_module("power-gzip_amd")
crb = importlib.import_module("power-gzip_amd.crb")

GUARD = 64                          # bytes behind every target that must stay as they were


@pytest.fixture(scope="module")
def eng():
    e = pkg.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def handle(eng):
    h = crb.DevHandle()
    assert eng.L.nx_function_begin(2, -1, C.byref(h)) == 0
    yield h
    eng.L.nx_function_end(C.byref(h))


class Batch:
    """jobs on the device: sources (each in a 16-byte aligned slot with room on either side, the job's src `front` bytes
    into it), targets filled with 0xAA, a dht_io slot per job"""

    def __init__(self, eng, items):
        """items: (front, source bytes, hist_len, dst_cap, resume, in_crc, in_adler, (dhtlen, table bytes) or None)"""
        import torch
        self.eng, self.n = eng, len(items)
        soff, doff, s, d = [], [], 0, 0
        for front, src, hist_len, cap, resume, crc, adler, dht in items:
            soff.append(s + 16 + front)
            s += (16 + front + len(src) + 32 + 15) & ~15
            doff.append(d)
            d += (cap + GUARD + 15) & ~15
        host = np.zeros(s + 16, np.uint8)
        for o, it in zip(soff, items):
            host[o:o + len(it[1])] = np.frombuffer(it[1], np.uint8)
        self.src = torch.from_numpy(host).to(eng.dev)
        self.dst = torch.empty(d + 16, dtype=torch.uint8, device=eng.dev)
        self.doff, self.caps = doff, [it[3] for it in items]
        j = np.zeros(self.n, pkg.JOB_DTYPE)
        j["src"] = np.uint64(self.src.data_ptr()) + np.array(soff, np.uint64)
        j["dst"] = np.uint64(self.dst.data_ptr()) + np.array(doff, np.uint64)
        assert self.src.data_ptr() % 16 == 0 and self.dst.data_ptr() % 16 == 0
        j["src_len"] = [len(it[1]) for it in items]
        j["hist_len"] = [it[2] for it in items]
        j["dst_cap"] = self.caps
        j["resume"] = [it[4] for it in items]
        j["in_crc"] = [it[5] for it in items]
        j["in_adler"] = [it[6] for it in items]
        self.jobs = eng.to_device(j)
        t = np.zeros(self.n, pkg.DHT_DTYPE)
        for i, it in enumerate(items):
            if it[7] is not None:
                t["dhtlen"][i] = it[7][0]
                t["dht"][i, :len(it[7][1])] = np.frombuffer(it[7][1], np.uint8)
        self.tables = t

    def run(self, with_tables=True):
        """-> (results, the targets as one host array, the dht_io slots afterwards)"""
        self.dst.fill_(0xAA)
        dht_io = self.eng.to_device(self.tables) if with_tables else None
        r = self.eng.results_to_host(self.eng.decompress(self.jobs, self.n, dht_io=dht_io))
        out = self.dst.cpu().numpy()
        return r, out, (dht_io.cpu().numpy().view(pkg.DHT_DTYPE) if with_tables else None)

    def target(self, out, i):
        """(the job's target, the guard behind it)"""
        o, cap = self.doff[i], self.caps[i]
        return out[o:o + cap], out[o + cap:o + cap + GUARD]


def item_of(c):
    front, src, hist_len = R.source_layout(c)
    dht = (c.dhtlen, c.dht[:288]) if (c.sfbt & 0xe) == 0xc else None
    return (front, src, hist_len, c.cap, R.resume_word(c), c.crc1, c.adler1, dht)


@pytest.fixture(scope="module")
def batch(eng):
    return Batch(eng, [item_of(c) for c in R.cases()])


def check_case(c, r, tgt, guard, slot, tag):
    """one job's result against the oracle's answer to the same input"""
    assert (guard == 0xAA).all(), tag                         # nothing beyond dst_cap
    if c.err:
        assert r["cc"] == c.err, (tag, r["cc"], c.err)
        return
    assert r["cc"] in (0, 3), (tag, r["cc"])
    assert r["tpbc"] == c.tpbc and tgt[:c.tpbc].tobytes() == c.out, tag
    subc = c.out_subc
    if c.final_eob and subc > 0xfff8:                         # SUBC is a 16-bit field: whole excess bytes stay unread
        subc -= 8 * ((subc - 0xfff8 + 7) // 8)
    assert (r["sfbt"] & 0xf) == c.out_sfbt and r["subc"] == subc, (tag, hex(r["sfbt"]), hex(c.out_sfbt), r["subc"], subc)
    assert bool(r["sfbt"] & 0x100) == c.final_eob, tag
    if (c.out_sfbt & 0xe) == 0x8:
        assert r["tebc"] == c.out_rem, (tag, r["tebc"], c.out_rem)
    if (c.out_sfbt & 0xe) == 0xc:
        nb = (c.out_dhtlen + 7) // 8
        assert slot["dhtlen"] == c.out_dhtlen and slot["dht"][:nb].tobytes() == c.out_dht[:nb], tag
    assert r["crc"] == zlib.crc32(c.out, c.crc1) and r["adler"] == zlib.adler32(c.out, c.adler1), tag


def check_batch(batch, res, route):
    r, out, dio = res
    for i, c in enumerate(R.cases()):
        tgt, guard = batch.target(out, i)
        check_case(c, r[i], tgt, guard, dio[i], (route, i, c.stream, c.k, c.m, c.layout, hex(c.sfbt), c.subc, c.rem))


@pytest.mark.parametrize("route", ROUTES)
def test_resumed_jobs_match_the_oracle(eng, batch, route):
    """every case as one batch: cc, tpbc, the bytes, where and how the job stopped again, the table it hands back, the
    checksums continued from the seeds, and nothing behind the target"""
    with inflate_route(route):
        res = batch.run()
    check_batch(batch, res, route)


def test_the_cut_route_twice_gives_the_same(eng, batch):
    """the round's table slots (a caller's table goes into one) are used again by the second call"""
    with inflate_route("cut"):
        a = batch.run()
        b = batch.run()
    check_batch(batch, a, "cut, first")
    check_batch(batch, b, "cut, second")
    for f in ("cc", "tpbc", "tebc", "spbc", "subc", "sfbt"):
        assert (a[0][f] == b[0][f]).all(), f
    ok = (a[0]["cc"] == 0) | (a[0]["cc"] == 3)
    assert (a[0]["crc"][ok] == b[0]["crc"][ok]).all() and (a[0]["adler"][ok] == b[0]["adler"][ok]).all()
    for i in np.nonzero(ok)[0]:
        n = int(a[0]["tpbc"][i])
        assert (batch.target(a[1], i)[0][:n] == batch.target(b[1], i)[0][:n]).all(), i


def _run_job_cases():
    """about 40 cases with their history whole, ten of every kind spread over the set; among them two that resume inside
    a dynamic block with 4096 bytes or more to go"""
    cs = [c for c in R.cases() if c.layout != "c" and c.err == 0 and c.m > 0]
    picked = []
    for kind in R.KINDS:
        v = [c for c in cs if (c.sfbt & 0xe) == kind]
        assert len(v) >= 10
        picked += [v[(i * len(v)) // 10] for i in range(10)]
    big = [c for c in cs if (c.sfbt & 0xe) == 0xc and len(c.part2) >= 4096]
    assert len(big) >= 2
    return picked + [big[0], big[-1]]


def test_nxu_run_job_resume_matches_model(eng, handle):
    """FC 0x14 through the transport symbol, source = the gather list [history, part 2], history a multiple of 16 bytes"""
    picked = _run_job_cases()
    for kind in R.KINDS:
        assert sum((c.sfbt & 0xe) == kind for c in picked) >= 5
    short = next(c for c in picked if (c.sfbt & 0xe) == 0x8 and c.tpbc > 1)
    for k, (c, dst) in enumerate([(c, [c.tpbc + 100] if i % 3 else [c.tpbc // 2, c.tpbc - c.tpbc // 2 + 100]) for i, c in enumerate(picked)] +
                                 [(short, [short.tpbc - 1])]):
        q = len(c.hist) // 16
        hist = c.hist[len(c.hist) - 16 * q:]
        kw = dict(fc=0x14, histlen_qw=q, in_crc=c.crc1, in_adler=c.adler1, subc=c.subc, sfbt=c.sfbt, rembytecnt=c.rem)
        if (c.sfbt & 0xe) == 0xc:
            kw.update(dht=c.dht[:288], dhtlen=c.dhtlen)
        dst = [n for n in dst if n > 0]
        gj, gd, cj, cd = run_both(eng, handle, kw, [hist, c.part2] if q else [c.part2], dst)
        tag = (k, c.stream, c.k, c.m, hex(c.sfbt))
        assert gj.cc == cj.cc and gj.ce3 == cj.ce3, (tag, gj.cc, cj.cc)
        if c is short and dst == [short.tpbc - 1]:
            assert cj.cc == 13
        if cj.cc in (0, 3):
            assert gj.tpbc == cj.tpbc and gd[:cj.tpbc] == cd[:cj.tpbc], tag
            assert (gj.out_sfbt, gj.out_subc, gj.out_spbc_decomp) == (cj.out_sfbt, cj.out_subc, cj.out_spbc_decomp), tag
            assert gj.out_crc == cj.out_crc and gj.out_adler == cj.out_adler, tag
            if (cj.out_sfbt & 0xe) == 0x8:
                assert gj.out_rembytecnt == cj.out_rembytecnt, tag
            if (cj.out_sfbt & 0xe) == 0xc:
                assert gj.out_dhtlen == cj.out_dhtlen, tag
                assert gj.out_dht[:(cj.out_dhtlen + 7) // 8] == cj.out_dht[:(cj.out_dhtlen + 7) // 8], tag


def _good_and_bad():
    """[(case or None, item)]: broken resume state, a good job on either side of each"""
    cs = R.cases()
    good = [c for c in cs if c.err == 0 and c.tpbc > 0 and c.m > 7]
    # (behind a 16-byte aligned start and long enough for the cut route to take it up: its plan copies the caller's table)
    dyn = min((c for c in good if c.forced and c.layout == "b" and len(c.part2) >= 2048), key=lambda c: len(c.part2))
    sto = next(c for c in good if (c.sfbt & 0xe) == 0x8 and c.rem < len(c.part2))
    front, src, hist_len = R.source_layout(dyn)

    def bad(dhtlen, table):
        return (front, src, hist_len, dyn.cap, R.resume_word(dyn), dyn.crc1, dyn.adler1, (dhtlen, table))

    bads = [bad(0, dyn.dht[:288]),                                            # a table of no bits
            bad(0xffffffff, b"\xff" * 292),                                   # a slot of 0xff bytes
            bad(dyn.dhtlen - 1, dyn.dht[:288]),                               # a table that parses to more bits than dhtlen says
            bad(dyn.dhtlen + 1, dyn.dht[:288])]                               # ... and to fewer
    # a stored block with more bytes to come than the source holds: what the oracle says (it suspends in the block)
    f2, s2, h2 = R.source_layout(sto)
    more = len(sto.part2) + 1000
    exp, st = O.inflate(sto.part2, sto.cap, hist=R.oracle_hist(sto) if sto.layout != "c" else b"", subc=0, sfbt=sto.sfbt, rembytecnt=more)
    long_rem = sto._replace(rem=more, err=st.err, out=exp, tpbc=st.tpbc, out_sfbt=st.out_sfbt, out_subc=st.out_subc, out_rem=st.out_rembytecnt,
                            final_eob=bool(st.final_eob))
    assert st.err in (0, 13) and (st.err or ((st.out_sfbt & 0xe) == 0x8 and st.out_rembytecnt == more - st.tpbc))
    items = []
    pool = [c for c in good if len(c.part2) < 4096][::7]
    for i, b in enumerate(bads):
        items += [(pool[2 * i], item_of(pool[2 * i])), (None, b)]
    items += [(pool[8], item_of(pool[8])), (long_rem, item_of(long_rem)), (pool[9], item_of(pool[9]))]
    return items


@pytest.mark.parametrize("route", ROUTES)
def test_broken_resume_state_is_refused_and_its_neighbours_stand(eng, route):
    """a job that resumes inside a dynamic block with a table that is empty, all ones or not dhtlen bits long, or in a batch
    without dht_io: NXZ_CC_INVALID_DHT, tpbc 0 and nothing written; the good jobs beside it are the oracle's"""
    pairs = _good_and_bad()
    b = Batch(eng, [it for _, it in pairs])
    with inflate_route(route):
        with_tables = b.run()
        without = b.run(with_tables=False)
    for i, (c, it) in enumerate(pairs):
        tag = (route, i)
        r, out, dio = with_tables
        tgt, guard = b.target(out, i)
        if c is None:
            assert r["cc"][i] == 68 and r["tpbc"][i] == 0, (tag, r[i])
            assert (tgt == 0xAA).all() and (guard == 0xAA).all(), tag
        else:
            check_case(c, r[i], tgt, guard, dio[i], tag)
        # no dht_io at all: every job that wants a table is refused, the others do not notice
        r, out, _ = without
        tgt, guard = b.target(out, i)
        if (it[4] >> 16 & 0xe) == 0xc:
            assert r["cc"][i] == 68 and r["tpbc"][i] == 0, (tag, r[i])
            assert (tgt == 0xAA).all() and (guard == 0xAA).all(), tag
        elif (c.out_sfbt & 0xe) != 0xc:                       # (a job that suspends inside a dynamic block has no slot to say so)
            check_case(c, r[i], tgt, guard, None, tag)
