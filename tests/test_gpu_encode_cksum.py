"""The block checksums of the function codes whose block the entropy kernel makes (nxz_encode.hip: the LZ77 kernel's
non-fused forms leave crc / adler of the result record to it).  The cases of cksum_grid -- lengths round the slice,
round, tile and block edges, histories, seeds, all-0xFF data -- as one batch per route: the device's own table
(DHTGEN, and the checked kernel form under NXZ_ENCODE_CHECK=1), a caller's table, the fixed code with symbol counts,
the shared dictionary calls, and a resume chain through nxu_run_job.  Every record is held against zlib over exactly
the non-history bytes AND against what the same jobs give through the fixed-code form in which the LZ77 kernel makes
the checksums itself."""
import ctypes as C
import importlib
import os
import zlib

import numpy as np
import pytest

import cksum_grid
import oracle_lib as O
from datagen import make_block

pytestmark = pytest.mark.gpu
pkg = importlib.import_module("power-gzip_amd")
crb = importlib.import_module("power-gzip_amd.crb")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RESUME = 0x08                                    # the function codes that take a history
KNOBS = ("NXZ_FUSED_GEN", "NXZ_COMPRESS_CHUNK", "NXZ_ENCODE_CHECK")


@pytest.fixture(scope="module")
def eng():
    saved = {k: os.environ.pop(k, None) for k in KNOBS}
    e = pkg.Engine(0)
    yield e
    e.close()
    for k, v in saved.items():
        if v is not None:
            os.environ[k] = v


def universal_table():
    """a caller's table with a code for every symbol"""
    b = make_block("alice", 20000, 3)
    tok, nt = O.lz77(b, 0)
    ll, d = O.counts(tok, nt)
    for i in range(286):
        ll[i] = max(ll[i], 1)
    for i in range(30):
        d[i] = max(d[i], 1)
    return O.dhtgen(ll, d)


def run_batch(eng, fc, cases, table=None, check=None, d=None):
    """the cases as one batch (every buffer at a 16-byte aligned place of one device tensor) -> result records.
    d: through nxz_batch_compress_dict (the cases have no history of their own then)"""
    import torch
    n = len(cases)
    at, total = [], 0
    for h, ln, _, _, buf in cases:
        at.append(total)
        total += (len(buf) + 16 + 15) & ~15
    host = np.full(max(total, 16), 0xa5, np.uint8)
    for a, c in zip(at, cases):
        host[a:a + len(c[4])] = np.frombuffer(c[4], np.uint8)
    src = torch.from_numpy(host).to(eng.dev)
    caps = np.array([int(eng.L.nxz_compress_bound(c[1])) + 512 for c in cases], np.uint64)
    dat = np.concatenate(([0], np.cumsum((caps + 31) & ~np.uint64(15))[:-1])).astype(np.uint64)
    dst = torch.zeros(int(dat[-1] + caps[-1] + 32), dtype=torch.uint8, device=eng.dev)
    j = np.zeros(n, pkg.JOB_DTYPE)
    j["src"] = np.uint64(src.data_ptr()) + np.array(at, np.uint64)
    j["dst"] = np.uint64(dst.data_ptr()) + dat
    j["src_len"] = [len(c[4]) for c in cases]
    j["hist_len"] = [c[0] for c in cases]
    j["dst_cap"] = caps
    j["in_crc"] = [c[2] for c in cases]
    j["in_adler"] = [c[3] for c in cases]
    jobs = eng.to_device(j)
    dht = None
    if table is not None:
        arr = np.zeros(1, pkg.DHT_DTYPE)
        arr["dhtlen"][0] = table[1]
        arr["dht"][0, :len(table[0])] = np.frombuffer(table[0], np.uint8)
        dht = eng.to_device(arr)
    if check is not None:
        os.environ["NXZ_ENCODE_CHECK"] = check
    try:
        if d is None:
            res, _ = eng.compress(fc, jobs, n, dht=dht, ntables=1 if table else 0)
        else:
            res, _ = eng.compress_dict(fc, d, jobs, n, dht=dht, ntables=1 if table else 0)
        return eng.results_to_host(res).copy()
    finally:
        os.environ.pop("NXZ_ENCODE_CHECK", None)


@pytest.fixture(scope="module")
def grid(eng):
    """(cases, zlib's checksums, the records of the fused fixed-code form), made once"""
    cases = cksum_grid.cases()
    exp = np.array([cksum_grid.expected(c) for c in cases], np.uint64)
    fused = run_batch(eng, pkg.FC_COMPRESS_FHT | RESUME, cases)
    return cases, exp, fused


def hold(r, cases, exp, fused, what):
    """crc / adler are zlib's; spbc, crc, adler are the fused form's"""
    bad = [(what, i, c[0], c[1], hex(c[2]), hex(c[3]), hex(int(r["crc"][i])), hex(int(e[0])), hex(int(r["adler"][i])), hex(int(e[1])))
           for i, (c, e) in enumerate(zip(cases, exp)) if int(r["crc"][i]) != e[0] or int(r["adler"][i]) != e[1]]
    assert not bad, (len(bad), bad[:8])
    for f in ("spbc", "crc", "adler"):
        diff = np.nonzero(r[f] != fused[f])[0]
        assert diff.size == 0, (what, f, diff[:8])


def test_the_fused_form_itself_equals_zlib(grid):
    cases, exp, fused = grid
    assert (fused["crc"] == exp[:, 0]).all() and (fused["adler"] == exp[:, 1]).all()
    assert (fused["spbc"] == [len(c[4]) for c in cases]).all()


@pytest.mark.parametrize("route", ["dhtgen", "dhtgen-checked", "dhtgen-count", "caller-table", "fht-count"])
def test_grid_through_every_non_fused_route(eng, grid, route):
    cases, exp, fused = grid
    if route == "dhtgen":
        r = run_batch(eng, pkg.FC_COMPRESS_DHTGEN | RESUME, cases, check="0")         # encode_kernel<true, false>
    elif route == "dhtgen-checked":
        r = run_batch(eng, pkg.FC_COMPRESS_DHTGEN | RESUME, cases, check="1")         # encode_kernel<true, true>
    elif route == "dhtgen-count":
        r = run_batch(eng, pkg.FC_COMPRESS_DHTGEN_COUNT | RESUME, cases)
    elif route == "caller-table":
        r = run_batch(eng, pkg.FC_COMPRESS_DHT | RESUME, cases, table=universal_table())
    else:
        r = run_batch(eng, pkg.FC_COMPRESS_FHT_COUNT | RESUME, cases)                 # encode_kernel<false, false>
    assert (r["cc"] != 66).all()
    hold(r, cases, exp, fused, route)


@pytest.mark.parametrize("dict_len", [5000, 32768])
def test_grid_through_the_dictionary_calls(eng, grid, dict_len):
    """a dictionary shorter than the window and one that fills it: the bytes below the source are the dictionary's,
    not the caller's, and no checksum may take them in"""
    text = open(os.path.join(ROOT, "tests", "golden", "alice29.txt"), "rb").read()
    d = eng.dict_create(text[:dict_len])
    try:
        W = d.deflate_window
        assert W == min(dict_len, 32768) & ~15
        cases = [c for c in grid[0] if c[0] == 0 and c[1] <= 65536 - W]
        assert len(cases) > 100 and max(c[1] for c in cases) >= 16384
        exp = np.array([cksum_grid.expected(c) for c in cases], np.uint64)
        fused = run_batch(eng, pkg.FC_COMPRESS_FHT, cases, d=d)
        assert (fused["crc"] == exp[:, 0]).all() and (fused["adler"] == exp[:, 1]).all()
        for fc in (pkg.FC_COMPRESS_DHTGEN, pkg.FC_COMPRESS_FHT_COUNT):
            r = run_batch(eng, fc, cases, d=d)
            hold(r, cases, exp, fused, "dict %d fc %#x" % (dict_len, fc))
    finally:
        d.close()


def test_a_resume_chain_of_three_parts_through_nxu_run_job(eng):
    """history carried (16-byte multiples), running checksums handed on: the last part's crc / adler are zlib's over
    the concatenation.  The three parts take the three forms of the entropy kernel."""
    h = crb.DevHandle()
    assert eng.L.nx_function_begin(2, -1, C.byref(h)) == 0
    try:
        table = universal_table()
        data = make_block("alice", 30000, 7) + b"\xff" * 9001 + make_block("lz", 20000, 8)
        cuts = [0, 30000 - 16 * 3, 30000 - 48 + 16 * 700 + 5, len(data)]
        assert cuts[1] % 16 == 0
        crc, adler, done = 0x1234, 77, 0
        seed_crc, seed_adler = crc, adler
        for k, fc in enumerate((0x0c, 0x0e, 0x2a)):
            part = data[cuts[k]:cuts[k + 1]]
            hist = data[max(0, done - 32768):done]
            hist = hist[len(hist) % 16:]
            j = crb.Job()
            srcs = [C.create_string_buffer(b, len(b)) for b in ([hist, part] if hist else [part])]
            dsts = [C.create_string_buffer(2 * len(part) + 1024)]
            kw = dict(fc=fc, histlen_qw=len(hist) // 16, in_crc=crc, in_adler=adler)
            if fc == 0x0e:
                kw.update(dht=table[0], dhtlen=table[1])
            j.setup(src_bufs=srcs, dst_bufs=dsts, **kw)
            assert eng.L.nxu_run_job(C.c_void_p(j.addr), C.byref(h)) == 0 and j.valid == 1
            assert j.cc in (0, 64), (k, j.cc)
            done += len(part)
            crc, adler = j.out_crc, j.out_adler
            assert crc == zlib.crc32(data[:done], seed_crc) and adler == zlib.adler32(data[:done], seed_adler), k
        assert done == len(data)
    finally:
        eng.L.nx_function_end(C.byref(h))
