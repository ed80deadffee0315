"""The LZ symbol counts of the function codes that count -- out_lzcount of the COUNT codes, the table generator's input of the
DHTGEN codes -- which nxzsc::count_kernel (nxz_symcount.hip) makes behind the LZ77 kernel's form that does not count.  Two
truths for every route: the oracle's counts of the block (symcount_cases.counts), and the same batch with
NXZ_LZ77_COUNT_INKERNEL=1, where the LZ77 kernel counts in its own out phase: counts equal word for word, and for DHTGEN
the output bytes and result records byte for byte.  The batch (symcount_cases.small_batch): every length round the lane's 8
positions, the bitmap word, the round of 2048, the LZ77 tile and the block; zeros (one length, one distance symbol), random
bytes (all literals), 33-symbol text, 0xff only, a block that uses every symbol; histories of 16 .. 32768 bytes (the
interface takes multiples of 16: histories of 1, 15 and 32767 bytes come as a dictionary of that length); every source
followed by bytes that are no zeros.  Then the batch in three chunks, the shared-dictionary calls, the one-stream deflate
with a dictionary (windowed first blocks plus the rest in one chunk) and nxu_run_job's round path."""
import ctypes as C
import importlib
import json
import os
import subprocess
import sys
import zlib
from contextlib import contextmanager

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":                       # the chunking test's child process: no conftest has set the path
    sys.path.insert(0, ROOT)

import oracle_lib as O
import symcount_cases as S
from datagen import make_block
from run_job import run_both

pytestmark = pytest.mark.gpu
pkg = importlib.import_module("power-gzip_amd")
crb = importlib.import_module("power-gzip_amd.crb")
RESUME = 0x08                                    # the function codes that take a history
KNOB = "NXZ_LZ77_COUNT_INKERNEL"
KNOBS = ("NXZ_FUSED_GEN", "NXZ_COMPRESS_CHUNK", "NXZ_ENCODE_CHECK", "NXZ_STREAMS_CHUNK", KNOB)
POISON = 0xa5


@pytest.fixture(scope="module")
def eng():
    saved = {k: os.environ.pop(k, None) for k in KNOBS}
    e = pkg.Engine(0)
    yield e
    e.close()
    for k, v in saved.items():
        if v is not None:
            os.environ[k] = v


@contextmanager
def inkernel(on):
    """the LZ77 kernel counts itself (the knob is read at every call)"""
    if on:
        os.environ[KNOB] = "1"
    try:
        yield
    finally:
        os.environ.pop(KNOB, None)


def universal_table():
    """a caller's table with a code for every symbol"""
    ll, d = O.counts(*O.lz77(make_block("alice", 20000, 3), 0))
    for i in range(286):
        ll[i] = max(ll[i], 1)
    for i in range(30):
        d[i] = max(d[i], 1)
    return O.dhtgen(ll, d)


def run_batch(eng, fc, cases, table=None, d=None, want_counts=True):
    """the cases as one batch, every buffer at a 16-byte aligned place of one device tensor of POISON bytes (so the 16 bytes
    and more behind every source are POISON) -> (result records, counts[n][316] or None, the outputs).
    d: through nxz_batch_compress_dict (the cases have no history of their own then)"""
    import torch
    n = len(cases)
    at, total = [], 0
    for _, data, _ in cases:
        at.append(total)
        total += (len(data) + 16 + 15) & ~15
    host = np.full(max(total, 16), POISON, np.uint8)
    for a, (_, data, _) in zip(at, cases):
        host[a:a + len(data)] = np.frombuffer(data, np.uint8)
    src = torch.from_numpy(host).to(eng.dev)
    caps = np.array([int(eng.L.nxz_compress_bound(len(data) - h)) + 512 for _, data, h in cases], np.uint64)
    dat = np.concatenate(([0], np.cumsum((caps + 31) & ~np.uint64(15))[:-1])).astype(np.uint64)
    dst = torch.zeros(int(dat[-1] + caps[-1] + 32), dtype=torch.uint8, device=eng.dev)
    j = np.zeros(n, pkg.JOB_DTYPE)
    j["src"] = np.uint64(src.data_ptr()) + np.array(at, np.uint64)
    j["dst"] = np.uint64(dst.data_ptr()) + dat
    j["src_len"] = [len(data) for _, data, _ in cases]
    j["hist_len"] = [h for _, _, h in cases]
    j["dst_cap"] = caps
    jobs = eng.to_device(j)
    dht = None
    if table is not None:
        arr = np.zeros(1, pkg.DHT_DTYPE)
        arr["dhtlen"][0] = table[1]
        arr["dht"][0, :len(table[0])] = np.frombuffer(table[0], np.uint8)
        dht = eng.to_device(arr)
    counts = torch.full((n * 316,), -1, dtype=torch.int32, device=eng.dev) if want_counts else None
    if d is None:
        res, _ = eng.compress(fc, jobs, n, dht=dht, ntables=1 if table else 0, counts=counts)
    else:
        res, _ = eng.compress_dict(fc, d, jobs, n, dht=dht, ntables=1 if table else 0, counts=counts)
    r = eng.results_to_host(res).copy()
    out = dst.cpu().numpy()
    outs = [out[int(a):int(a) + int(t)].tobytes() for a, t in zip(dat, r["tpbc"])]
    cnt = counts.cpu().numpy().view(np.uint32).reshape(n, 316) if want_counts else None
    return r, cnt, outs


@pytest.fixture(scope="module")
def batch():
    """(cases, the oracle's counts), made once"""
    cases = S.small_batch()
    return cases, np.stack([S.counts(data, h) for _, data, h in cases])


def hold_counts(cnt, cases, truth, what):
    bad = [(what, name, len(data), h, np.nonzero(c != t)[0][:6].tolist()) for (name, data, h), c, t in zip(cases, cnt, truth) if (c != t).any()]
    assert not bad, (len(bad), bad[:6])


@pytest.mark.parametrize("route", ["caller-table", "dhtgen", "fixed"])
def test_counts_of_the_small_batch_are_the_oracle_s_and_the_in_kernel_form_s(eng, batch, route):
    cases, truth = batch
    fc = {"caller-table": pkg.FC_COMPRESS_DHT_COUNT, "dhtgen": pkg.FC_COMPRESS_DHTGEN_COUNT, "fixed": pkg.FC_COMPRESS_FHT_COUNT}[route] | RESUME
    table = universal_table() if route == "caller-table" else None
    r, cnt, outs = run_batch(eng, fc, cases, table=table)
    hold_counts(cnt, cases, truth, route)
    with inkernel(True):
        r1, cnt1, outs1 = run_batch(eng, fc, cases, table=table)
    hold_counts(cnt1, cases, truth, route + " in-kernel")
    assert (cnt == cnt1).all() and r.tobytes() == r1.tobytes() and outs == outs1


def test_dhtgen_without_a_count_code_gives_the_oracle_s_block_and_the_in_kernel_form_s_bytes(eng, batch):
    cases, truth = batch
    fc = pkg.FC_COMPRESS_DHTGEN | RESUME
    r, _, outs = run_batch(eng, fc, cases, want_counts=False)
    with inkernel(True):
        r1, _, outs1 = run_batch(eng, fc, cases, want_counts=False)
    assert r.tobytes() == r1.tobytes() and outs == outs1
    assert np.isin(r["cc"], (0, 64)).all(), r["cc"]
    for (name, data, h), rec, got in zip(cases, r, outs):
        ll, d = O.counts(*O.lz77(data, h))
        exp, bits = O.deflate_dynamic(data, *O.dhtgen(ll, d), hist=h)
        assert got == exp and rec["tebc"] == bits % 8, name
        inflater = zlib.decompressobj(-15, zdict=data[:h]) if h else zlib.decompressobj(-15)
        assert inflater.decompress(got) == data[h:], name


def _chunk_child():
    """600 jobs of 4 KiB (run with NXZ_COMPRESS_CHUNK=256: three chunks of 200): the counts as a JSON list of 600 x 316"""
    e = pkg.Engine(0)
    cases = [("c%d" % i, make_block(("alice", "lz", "text33", "random")[i % 4], 4096, seed=i), 0) for i in range(600)]
    _, cnt, _ = run_batch(e, pkg.FC_COMPRESS_DHTGEN_COUNT, cases)
    e.close()
    print("COUNTS " + json.dumps(cnt.tolist()))


def test_counts_of_job_i_stand_at_i_times_316_across_three_chunks(eng):
    """the chunk size is read once a process: a process of its own"""
    env = dict(os.environ, NXZ_COMPRESS_CHUNK="256")
    env.pop(KNOB, None)
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--chunk-child"], env=env, capture_output=True, text=True, timeout=300)
    line = [x for x in p.stdout.splitlines() if x.startswith("COUNTS ")]
    assert p.returncode == 0 and line, (p.returncode, p.stderr[-2000:])
    cnt = np.array(json.loads(line[0][7:]), np.uint32)
    assert cnt.shape == (600, 316)
    for i in range(600):
        t = S.counts(make_block(("alice", "lz", "text33", "random")[i % 4], 4096, seed=i))
        assert (cnt[i] == t).all(), i


def test_the_shared_dictionary_calls(eng):
    """nxz_batch_compress_dict with a 4 KiB dictionary: the window is the dictionary's, the counts the source's alone"""
    text = open(os.path.join(ROOT, "tests", "golden", "alice29.txt"), "rb").read()
    dic = text[1000:1000 + 4096]
    d = eng.dict_create(dic)
    try:
        W = d.deflate_window
        assert W == 4096
        sources = [text[9000:9000 + n] for n in (0, 1, 9, 2049, 16385, 60000)] + [make_block("random", 3000, 1), bytes(5000), b"\xff" * 33]
        cases = [("dict/%d" % i, s, 0) for i, s in enumerate(sources)]
        truth = np.stack([S.counts(dic[-W:] + s, W) for s in sources])
        for fc in (pkg.FC_COMPRESS_DHTGEN_COUNT, pkg.FC_COMPRESS_FHT_COUNT):
            r, cnt, outs = run_batch(eng, fc, cases, d=d)
            hold_counts(cnt, cases, truth, "dict fc %#x" % fc)
            with inkernel(True):
                r1, cnt1, outs1 = run_batch(eng, fc, cases, d=d)
            assert (cnt == cnt1).all() and r.tobytes() == r1.tobytes() and outs == outs1
    finally:
        d.close()


@pytest.mark.parametrize("hist", S.DICT_HISTORIES)
def test_histories_that_are_no_multiple_of_16_as_a_dictionary(eng, hist):
    """the batched interface takes hist_len in multiples of 16 only (include/nxz_engine.h); a history of 1, 15 or 32767 bytes
    is a dictionary of that length, of which the last W = min(len, 32768) & ~15 bytes are every job's window"""
    data = make_block("alice", hist + 30000, seed=70) if hist < 100 else make_block("lz", 65536 - 16, seed=71)
    dic = data[:hist]
    d = eng.dict_create(dic)
    try:
        W = d.deflate_window
        assert W == min(hist, 32768) & ~15
        sources = [data[hist:], data[hist:hist + 2049], b"\xff" * 9]
        sources = [s[:65536 - W] for s in sources]
        cases = [("dict-history/%d/%d" % (hist, i), s, 0) for i, s in enumerate(sources)]
        truth = np.stack([S.counts(dic[hist - W:] + s, W) for s in sources])
        r, cnt, outs = run_batch(eng, pkg.FC_COMPRESS_DHTGEN_COUNT, cases, d=d)
        hold_counts(cnt, cases, truth, "dictionary of %d" % hist)
        with inkernel(True):
            r1, cnt1, outs1 = run_batch(eng, pkg.FC_COMPRESS_DHTGEN_COUNT, cases, d=d)
        assert (cnt == cnt1).all() and r.tobytes() == r1.tobytes() and outs == outs1
    finally:
        d.close()


def test_one_stream_deflate_with_a_dictionary_windowed_first_blocks_and_the_rest(eng):
    """nxz_batch_deflate_streams_dict on two streams of 100 KiB: the chunk's two first blocks take the dictionary's window
    (lz77_dict_kernel), its other blocks their own history (lz77_kernel) -- the counts of both launches in one array"""
    import torch
    text = open(os.path.join(ROOT, "tests", "golden", "alice29.txt"), "rb").read()
    dic = text[:4096]
    datas = [text[5000:5000 + 102400], make_block("lz", 102400, seed=9)]
    d = eng.dict_create(dic)
    try:
        bufs = [torch.from_numpy(np.frombuffer(x, np.uint8).copy()).to(eng.dev) for x in datas]
        got = []
        for on in (False, True):
            with inkernel(on):
                out, offsets, results = eng.deflate_streams_dict(pkg.FC_COMPRESS_DHTGEN, pkg.FMT_ZLIB, d, bufs, hist_max=32768)
                r = eng.results_to_host(results, pkg.engine.STREAM_RESULT_DTYPE).copy()
            o = out.cpu().numpy()
            got.append((r, [o[int(offsets[i]):int(offsets[i]) + int(r["out_len"][i])].tobytes() for i in range(2)]))
        assert (got[0][0]["cc"] == 0).all() and got[0][0].tobytes() == got[1][0].tobytes() and got[0][1] == got[1][1]
        for x, s in zip(datas, got[0][1]):
            assert zlib.decompressobj(zdict=dic).decompress(s) == x
    finally:
        d.close()


def test_nxu_run_job_s_round_path_with_a_count_code(eng):
    """the counts lie in the job's parameter block, in host memory the device writes to"""
    h = crb.DevHandle()
    assert eng.L.nx_function_begin(2, -1, C.byref(h)) == 0
    try:
        body = make_block("alice", 30000, 2)
        table = universal_table()
        for fc, kw in ((0x04, {}), (0x06, dict(dht=table[0], dhtlen=table[1]))):
            for on in (False, True):
                with inkernel(on):
                    gj, gd, cj, cd = run_both(eng, h, dict(fc=fc, histlen_qw=0, in_crc=0, in_adler=1, **kw), [body], [70000])
                assert gj.cc == cj.cc == 0 and gj.tpbc == cj.tpbc and gd[:cj.tpbc] == cd[:cj.tpbc]
                assert gj.lzcounts == cj.lzcounts and gj.out_spbc_count == cj.out_spbc_count
                assert gj.lzcounts == S.counts(body).tolist()
    finally:
        eng.L.nx_function_end(C.byref(h))


if __name__ == "__main__" and sys.argv[1:] == ["--chunk-child"]:
    _chunk_child()
