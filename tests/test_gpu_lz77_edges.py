"""The LZ77 kernel (power-gzip_amd/csrc/nxz_lz77.hip) on the edge-case set of tests/lz77_cases.py, through every form it is
built in -- fused fixed code, tokens for a caller's table (with and without counts), tokens for a table of the block's own
(three kernels and NXZ_FUSED_GEN=1), the RESUME codes with history and running checksums, and the dictionary form --, bit for
bit against oracle/nxz_lz77.c.  tests/test_lz77_cases_host.py shows on the CPU that the set reaches the regime switches (first
tile's token count at 3071 / 3072 / 3073, 1023 / 1024 bytes >= 0x80) and the numeric edges (distance 32768, LAZY_MAX, the piece
lag of second entries, tile-end truncation, the 12-byte run rule) and that a wrong constant changes the tokens.

A launch holds the set several times over, in one order and reversed: more jobs than CUs, so a persistent workgroup takes a
text block behind a bin-hard one and the other way round (stale first-tile state, second entries of the job before).

The batched interface takes histories that are a multiple of 16 (include/nxz_engine.h); the cases with other history lengths
reach the device through nxz_batch_compress_dict, which rounds the window down to 16 (nxz_dict.h), and are compared with the
oracle on [window][source]."""
import importlib
import json
import os
import zlib

import numpy as np
import pytest

import lz77_cases as Z
import oracle_lib as O

pytestmark = pytest.mark.gpu
pkg = importlib.import_module("power-gzip_amd")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRIDE_IN = 65536
STRIDE_OUT = 2 * 65536 + 2048        # a caller's table may code a literal in 15 bits
REPEAT = 3                           # 3 x the set: more jobs than the device has CUs
IN_CRC, IN_ADLER = 0x1234abcd, 0x00c0ffee
KNOBS = ("NXZ_FUSED_GEN", "NXZ_COMPRESS_CHUNK")


@pytest.fixture(scope="module")
def eng():
    saved = {k: os.environ.pop(k, None) for k in KNOBS}
    e = pkg.Engine(0)
    yield e
    e.close()
    for k, v in saved.items():
        if v is not None:
            os.environ[k] = v


def _universal_table():
    """every symbol has a code (shaped after a mix of the set's own counts)"""
    ll = (O.C.c_uint32 * 286)(*([1] * 286))
    d = (O.C.c_uint32 * 30)(*([1] * 30))
    for name in ("bin-hard/32768", "text-threshold/32768/1023", "window/block/32768"):
        tok, nt = O.lz77(*[(c[1], c[2]) for c in Z.all_cases() if c[0] == name][0])
        cl, cd = O.counts(tok, nt)
        for i in range(286):
            ll[i] += cl[i]
        for i in range(30):
            d[i] += cd[i]
    return O.dhtgen(ll, d)


@pytest.fixture(scope="module")
def tables():
    g = json.load(open(os.path.join(ROOT, "tests", "golden", "builtin_dht.json")))
    # a canned table, one with every code, and the exact table of one text block (most other blocks miss a code under it: CC 66)
    tok, nt = O.lz77(*[(c[1], c[2]) for c in Z.all_cases() if c[0] == "text-threshold/20000/1023"][0])
    return [(bytes.fromhex(g[0]["dht"]), g[0]["dhtlen"]), _universal_table(), O.dhtgen(*O.counts(tok, nt))]


_expected = {}


def expected(data, hist, table=None):
    """the oracle's block for data[hist:] behind data[:hist]: (bytes or None, bits, counts); table None: fixed code, "own": the
    block's own table, else a caller's table.  Computed once per (block, table)."""
    key = (data, hist, table)
    if key not in _expected:
        tok, nt = O.lz77(data, hist)
        ll, d = O.counts(tok, nt)
        cnt = np.array(list(ll) + list(d), np.uint32)
        if table is None:
            out, bits = O.deflate_fixed(data, hist)
        else:
            dht, dhtlen = O.dhtgen(ll, d) if table == "own" else table
            cap = 2 * len(data) + 2048
            buf = O.C.create_string_buffer(cap)
            bits = O.lib().nxo_encode_dynamic(tok, nt, dht, dhtlen, buf, cap)
            out = buf.raw[:(bits + 7) // 8] if bits < (1 << 62) else None
        _expected[key] = (out, bits, cnt)
    return _expected[key]


def launch(eng, fc, jobs_in, tabs=None, in_crc=0, in_adler=1, dictionary=None):
    """jobs_in: [(data, hist, table index)] -> (results, output rows, counts or None)"""
    import torch
    n = len(jobs_in)
    off = [h if dictionary is not None else 0 for _, h, _ in jobs_in]        # (a dictionary job is the source alone)
    host = np.zeros((n, STRIDE_IN), np.uint8)
    for i, (d, h, _) in enumerate(jobs_in):
        host[i, :len(d) - off[i]] = np.frombuffer(d, np.uint8)[off[i]:]
    src = torch.from_numpy(host).to(eng.dev)
    dst = torch.zeros((n, STRIDE_OUT), dtype=torch.uint8, device=eng.dev)
    lens = np.array([len(d) - o for (d, _, _), o in zip(jobs_in, off)], np.uint32)
    hl = np.array([0 if dictionary is not None else h for _, h, _ in jobs_in], np.uint32)
    assert not (hl % 16).any() and (lens <= STRIDE_IN).all()
    jobs = eng.jobs_strided(src, STRIDE_IN, lens, dst, STRIDE_OUT, STRIDE_OUT, hist_len=hl, in_crc=in_crc, in_adler=in_adler,
                            dht_index=np.array([t or 0 for _, _, t in jobs_in], np.uint32))
    dht = None
    if tabs:
        arr = np.zeros(len(tabs), pkg.DHT_DTYPE)
        for i, (bits, nb) in enumerate(tabs):
            arr["dhtlen"][i] = nb
            arr["dht"][i, :len(bits)] = np.frombuffer(bits, np.uint8)
        dht = eng.to_device(arr)
    if dictionary is not None:
        res, cnt = eng.compress_dict(fc, dictionary, jobs, n, dht=dht, ntables=len(tabs or ()))
    else:
        res, cnt = eng.compress(fc, jobs, n, dht=dht, ntables=len(tabs or ()))
    r = eng.results_to_host(res).copy()
    out = dst.cpu().numpy()
    cnt = cnt.cpu().numpy().view(np.uint32).reshape(n, 316) if cnt is not None else None
    return r, out, cnt


def check(fc, jobs_in, names, r, out, cnt, tabs=None, in_crc=0, in_adler=1, window=None):
    """every job against the oracle, exactly: bytes, tpbc, tebc, spbc, both checksums, the completion code, and zlib's inflate"""
    for i, ((data, hist, ti), name) in enumerate(zip(jobs_in, names)):
        table = None if not fc & 0x22 else "own" if fc & 0x20 else tabs[ti]
        if window is not None:                                   # the dictionary form: [deflate window][source]
            body = data[hist:]
            data, hist = window + body, len(window)
        exp, bits, ocnt = expected(data, hist, table)
        body = data[hist:]
        where = (name, i, hex(fc))
        if exp is None:                                          # the caller's table has no code for a symbol of this block
            assert r["cc"][i] == 66, where
            continue
        assert r["tpbc"][i] == len(exp) and r["tebc"][i] == bits % 8, where + (int(r["cc"][i]), int(r["tpbc"][i]), len(exp))
        assert out[i, :len(exp)].tobytes() == exp, where
        assert r["spbc"][i] == (len(body) if window is not None else len(data)), where
        assert r["crc"][i] == zlib.crc32(body, in_crc) and r["adler"][i] == zlib.adler32(body, in_adler), where
        assert r["cc"][i] == (64 if len(exp) > len(data) else 0), where
        if fc & 0x4:
            assert (cnt[i] == ocnt).all(), where
        z = zlib.decompressobj(-15, zdict=data[:hist]) if hist else zlib.decompressobj(-15)
        assert z.decompress(out[i, :len(exp)].tobytes()) == body and z.eof, where


def both_orders(cases):
    base = list(cases) * REPEAT
    return [base, base[::-1]]


FORMS = [("FHT", {}), ("DHT", {}), ("DHT_COUNT", {}), ("DHTGEN", {"NXZ_FUSED_GEN": "0"}), ("DHTGEN", {"NXZ_FUSED_GEN": "1"}),
         ("DHTGEN_COUNT", {})]


@pytest.mark.parametrize("form,env", FORMS, ids=[f + "".join("-%s=%s" % kv for kv in e.items()) for f, e in FORMS])
def test_edge_set_without_history(eng, tables, form, env):
    fc = getattr(pkg, "FC_COMPRESS_" + form)
    cases = [c for c in Z.all_cases() if c[2] == 0]
    caller = bool(fc & 0x2) and not fc & 0x20
    os.environ.update(env)
    try:
        for order in both_orders(cases):
            # a caller's table: every block under each of the three
            jobs_in = [(d, h, t) for _, d, h in order for t in ((0, 1, 2) if caller else (None,))]
            names = [nm for nm, _, _ in order for _ in ((0, 1, 2) if caller else (None,))]
            r, out, cnt = launch(eng, fc, jobs_in, tables if caller else None)
            check(fc, jobs_in, names, r, out, cnt, tables)
    finally:
        for k in env:
            os.environ.pop(k, None)


@pytest.mark.parametrize("form", ["RESUME_FHT", "RESUME_DHT_COUNT", "RESUME_DHTGEN"])
def test_edge_set_with_history_and_running_checksums(eng, tables, form):
    """every case whose history the interface takes (a multiple of 16: none, 16, 32768), the histories of
    tests/lz77_cases.history() among them"""
    fc = getattr(pkg, "FC_COMPRESS_" + form)
    cases = [c for c in Z.all_cases() if c[2] % 16 == 0]
    assert {c[2] for c in cases} == {0, 16, 32768} and sum(1 for c in cases if c[2]) >= 10
    caller = not fc & 0x20 and bool(fc & 0x2)
    for order in both_orders(cases):
        jobs_in = [(d, h, 1 if caller else None) for _, d, h in order]
        r, out, cnt = launch(eng, fc, jobs_in, tables if caller else None, IN_CRC, IN_ADLER)
        check(fc, jobs_in, [c[0] for c in order], r, out, cnt, tables, IN_CRC, IN_ADLER)


@pytest.mark.parametrize("form", ["FHT", "DHTGEN_COUNT"])
def test_edge_set_behind_a_shared_dictionary(eng, form):
    """window-edge, run-edge and history cases with their history as the dictionary: nxz_batch_compress_dict takes its last
    W = min(len, 32768) & ~15 bytes as every job's window -- histories of 1 .. 32767 bytes reach the kernel as 0, 16, 4080, 32752"""
    fc = getattr(pkg, "FC_COMPRESS_" + form)
    cases = [c for c in Z.all_cases() if c[2] and c[0].startswith(("window/", "run/", "history/"))]
    assert {c[2] for c in cases} >= {1, 4, 8, 15, 16, 17, 4095, 32767, 32768}
    for name, data, hist in cases:
        d = eng.dict_create(data[:hist])
        try:
            W = d.deflate_window
            assert W == min(hist, 32768) & ~15
            jobs_in = [(data, hist, None)] * REPEAT
            r, out, cnt = launch(eng, fc, jobs_in, dictionary=d)
            check(fc, jobs_in, [name] * REPEAT, r, out, cnt, window=data[hist - W:hist])
        finally:
            d.close()
