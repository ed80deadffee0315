"""The hand-built streams of tests/deflate_handmade.py through every inflate route of nxz_batch_decompress and through the
size and verify calls: one batch a call, every record and every byte against the CPU oracle's answer to the same stream
(tests/test_deflate_handmade_host.py holds that answer to zlib).  No tolerance, no case left out on any route: a stream a
kernel hands on to another kernel is that route's business, its record is checked all the same."""
import importlib
import zlib

import numpy as np
import pytest

import deflate_handmade as H
from inflate_routes import ROUTES, inflate_route
from test_gpu_inflate_resume import GUARD, Batch, check_case
from test_gpu_size import check_against_oracle, make_jobs, place

pytestmark = pytest.mark.gpu
pkg = importlib.import_module("power-gzip_amd")


@pytest.fixture(scope="module")
def eng():
    e = pkg.Engine(0)
    yield e
    e.close()


def front(i):
    return (5 * i) % 16


@pytest.fixture(scope="module")
def batches(eng):
    """{copies: Batch}: the set once (187 jobs) and three times over (more than a wavefront of jobs a lane route)"""
    recs = H.records()
    assert GUARD == 64
    return {k: Batch(eng, [(front(i), c.hist + c.src, len(c.hist), c.cap, 0, c.crc1, c.adler1, None)
                           for i, c in enumerate(recs * k)]) for k in (1, 3)}


@pytest.mark.parametrize("copies", [1, 3])
@pytest.mark.parametrize("route", ROUTES)
def test_every_route_takes_the_oracles_verdict(eng, batches, route, copies):
    """cc, tpbc, the bytes, where and how a job stopped (sfbt, subc, tebc, the table handed back), the final-EOB bit, both
    checksums, and the 64 bytes behind every target as they were"""
    recs, b = H.records() * copies, batches[copies]
    with inflate_route(route):
        r, out, dio = b.run()
    for i, c in enumerate(recs):
        tgt, guard = b.target(out, i)
        check_case(c, r[i], tgt, guard, dio[i], (route, i, c.name))


@pytest.mark.parametrize("call", ["size", "verify"])
def test_size_and_verify_take_the_oracles_verdict(eng, call):
    recs = H.records()
    bufs = [c.hist + c.src for c in recs]
    src, addrs = place(eng, bufs, [front(i) for i in range(len(recs))])
    jobs = eng.to_device(make_jobs(addrs, [len(b) for b in bufs], [c.cap for c in recs], hist=[len(c.hist) for c in recs]))
    r = eng.results_to_host((eng.decompress_size if call == "size" else eng.decompress_verify)(jobs, len(recs))).copy()
    for i, c in enumerate(recs):
        if call == "verify" and int(r["cc"][i]) in (0, 3):  # (the checksums here, the rest of the record as the size call's)
            assert int(r["crc"][i]) == zlib.crc32(c.out) and int(r["adler"][i]) == zlib.adler32(c.out), c.name
            r["crc"][i] = r["adler"][i] = 0
        try:
            check_against_oracle(r, i, c.src, c.cap, hist=c.hist)
        except AssertionError as e:
            raise AssertionError("%s: %s" % (c.name, e)) from None
