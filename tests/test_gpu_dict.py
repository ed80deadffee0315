"""GPU tests of the shared preset dictionary of the batched interface (include/nxz_engine.h: nxz_dict_create,
nxz_batch_compress_dict, nxz_batch_decompress_dict, nxz_batch_pack_zlib_dict, nxz_batch_decompress_framed_dict; the rules in
power-gzip_amd/csrc/nxz_dict.h).  Three references: the CPU oracle on [window][data], the engine's own plain calls on jobs staged
as [window][data] with hist_len (what a caller had to do before), and system zlib with zdict= (an independent implementation)."""
import ctypes as C
import functools
import importlib
import json
import os
import struct
import zlib

import numpy as np
import pytest

import framing as F
import oracle_lib as O
from datagen import make_block

pytestmark = pytest.mark.gpu
pkg = importlib.import_module("power-gzip_amd")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CC_OK, CC_DATA_LENGTH, CC_INVALID_OP, CC_TARGET_SPACE, CC_INVALID_DIST = 0, 3, 8, 13, 67   # include/nxz_engine.h NXZ_CC_*
KNOBS = ("NXZ_INFLATE_LANES_MIN", "NXZ_INFLATE_CUT", "NXZ_INFLATE_WG", "NXZ_INFLATE_WG_MAX", "NXZ_WG_PMIN", "NXZ_INFLATE_ORDER",
         "NXZ_FUSED_GEN", "NXZ_COMPRESS_CHUNK", "NXZ_DICT_WG_MIN")
DICT_LENS = [0, 1, 15, 16, 17, 100, 32767, 32768, 32769, 40000, 100000]
TEXT = open(os.path.join(ROOT, "tests", "golden", "alice29.txt"), "rb").read()


@pytest.fixture(scope="module")
def eng():
    saved = {k: os.environ.pop(k, None) for k in KNOBS}
    e = pkg.Engine(0)
    yield e
    e.close()
    for k, v in saved.items():
        if v is not None:
            os.environ[k] = v


@pytest.fixture(params=["by size", "workgroup"])
def route(request):
    """nxz_batch_decompress_dict's routes: streams below NXZ_DICT_WG_MIN source bytes a wavefront each (the default), or every
    stream through the workgroup kernel with the preloaded window (NXZ_DICT_WG_MIN=0)"""
    if request.param == "workgroup":
        os.environ["NXZ_DICT_WG_MIN"] = "0"
    yield request.param
    os.environ.pop("NXZ_DICT_WG_MIN", None)


def jsonish(n, seed):
    rows, i = [], seed * 1000
    while sum(map(len, rows)) < n:
        rows.append(b'{"id": %d, "name": "user%d", "active": %s, "tags": ["a%d", "b"], "score": %d.%d}\n'
                    % (i, i % 97, b"true" if i % 3 else b"false", i % 7, i * 31 % 1000, i % 10))
        i += 1
    return b"".join(rows)[:n]


def make_dict(n):
    """n bytes the records below share vocabulary with: text, then JSON-like rows"""
    d = TEXT[:n // 2] + jsonish(n - n // 2, 7)
    assert len(d) == n
    return d


def record(kind, n, seed):
    if kind == "text":
        at = (seed * 7919) % (len(TEXT) - n) if n < len(TEXT) else 0
        return TEXT[at:at + n]
    if kind == "json":
        return jsonish(n, seed)
    return make_block(kind, n, seed=seed)


def place(eng, bufs, offs=None, fill=0xa5):
    """bufs in one device tensor, each at a 16-byte aligned place (+ offs[i]); returns (tensor, device addresses)"""
    import torch
    offs = offs or [0] * len(bufs)
    at, total = [], 0
    for b, o in zip(bufs, offs):
        at.append(total + o)
        total += (o + len(b) + 16 + 15) & ~15
    host = np.full(max(total, 16), fill, np.uint8)
    for b, a in zip(bufs, at):
        host[a:a + len(b)] = np.frombuffer(b, np.uint8)
    t = torch.from_numpy(host).to(eng.dev)
    return t, np.uint64(t.data_ptr()) + np.array(at, np.uint64)


def targets(eng, caps, sentinel=0xcd, offs=None):
    import torch
    at, total = [], 0
    for i, c in enumerate(caps):
        o = offs[i] if offs else 0
        at.append(total + o)
        total += (o + c + 16 + 15) & ~15
    t = torch.full((max(total, 16),), sentinel, dtype=torch.uint8, device=eng.dev)
    return t, np.array(at, np.int64)


def make_jobs(eng, src_addr, src_lens, dst_t, dst_at, caps, hist_len=0, dht_index=None, reserved=0):
    n = len(src_lens)
    j = np.zeros(n, pkg.JOB_DTYPE)
    j["src"] = src_addr
    j["dst"] = np.uint64(dst_t.data_ptr()) + dst_at.astype(np.uint64)
    j["src_len"] = src_lens
    j["hist_len"] = hist_len
    j["dst_cap"] = caps
    j["in_adler"] = 1
    j["reserved"] = reserved
    if dht_index is not None:
        j["dht_index"] = dht_index
    return eng.to_device(j)


def _dht_array(tables):
    arr = np.zeros(len(tables), pkg.DHT_DTYPE)
    for i, (bits, n) in enumerate(tables):
        arr["dhtlen"][i] = n
        arr["dht"][i, :len(bits)] = np.frombuffer(bits, np.uint8)
    return arr


def builtin_table():
    g = json.load(open(os.path.join(ROOT, "tests", "golden", "builtin_dht.json")))
    return bytes.fromhex(g[0]["dht"]), g[0]["dhtlen"]


def oracle_block(fc, data, W, table):
    """(bytes, bits, counts) of the oracle for [window][source] with hist = W"""
    tok, nt = O.lz77(data, W)
    ll, d = O.counts(tok, nt)
    cnt = np.array(list(ll) + list(d), np.uint32)
    if not fc & 0x22:
        out, bits = O.deflate_fixed(data, hist=W)
        return out, bits, cnt
    if fc & 0x20:
        dht, dhtlen = O.dhtgen(ll, d)
    else:
        dht, dhtlen = table
    cap = 2 * len(data) + 2048
    buf = C.create_string_buffer(cap)
    bits = O.lib().nxo_encode_dynamic(tok, nt, dht, dhtlen, buf, cap)
    assert bits < (1 << 62)
    return buf.raw[:(bits + 7) // 8], bits, cnt


def compress_both(eng, d, dict_bytes, sources, fc, table=None):
    """the sources through compress_dict and, staged as [deflate window][source] with hist_len = W, through compress"""
    W = d.deflate_window
    window = dict_bytes[len(dict_bytes) - W:]
    n = len(sources)
    caps = [int(eng.L.nxz_compress_bound(len(s))) + 512 for s in sources]
    lens = np.array([len(s) for s in sources], np.uint32)
    dht = eng.to_device(_dht_array([table])) if table else None
    nt = 1 if table else 0
    st, saddr = place(eng, sources)
    dt, dat = targets(eng, caps)
    res, cnt = eng.compress_dict(fc, d, make_jobs(eng, saddr, lens, dt, dat, caps), n, dht=dht, ntables=nt)
    r = eng.results_to_host(res).copy()
    out = dt.cpu().numpy()
    cnt = cnt.cpu().numpy().view(np.uint32).reshape(n, 316) if cnt is not None else None
    st2, saddr2 = place(eng, [window + s for s in sources])
    dt2, dat2 = targets(eng, caps)
    res2, cnt2 = eng.compress(fc, make_jobs(eng, saddr2, lens + np.uint32(W), dt2, dat2, caps, hist_len=W), n, dht=dht, ntables=nt)
    r2 = eng.results_to_host(res2).copy()
    out2 = dt2.cpu().numpy()
    cnt2 = cnt2.cpu().numpy().view(np.uint32).reshape(n, 316) if cnt2 is not None else None
    return (r, out, cnt, dat), (r2, out2, cnt2, dat2), window


def check_compress(eng, dict_bytes, sources, fc, oracle_every=1):
    d = eng.dict_create(dict_bytes)
    try:
        assert d.id == zlib.adler32(dict_bytes)
        W = d.deflate_window
        assert W == min(len(dict_bytes), 32768) & ~15
        table = builtin_table() if fc == pkg.FC_COMPRESS_DHT_COUNT else None
        (r, out, cnt, dat), (r2, out2, cnt2, _), window = compress_both(eng, d, dict_bytes, sources, fc, table)
        # the staged layout through the plain call: everything but spbc, which counts the source alone here
        lens = np.array([len(s) for s in sources], np.uint32)
        for f in ("cc", "tpbc", "tebc", "crc", "adler", "subc", "sfbt"):
            assert (r[f] == r2[f]).all(), (f, np.nonzero(r[f] != r2[f])[0][:8])
        assert (r["spbc"] == lens).all() and (r2["spbc"] == lens + np.uint32(W)).all()
        assert np.isin(r["cc"], (0, 64)).all(), r["cc"][~np.isin(r["cc"], (0, 64))][:8]
        if cnt is not None:
            assert (cnt == cnt2).all()
        for i, s in enumerate(sources):
            a, k = int(dat[i]), int(r["tpbc"][i])
            got = out[a:a + k].tobytes()
            assert got == out2[a:a + k].tobytes(), i
            assert r["crc"][i] == zlib.crc32(s) and r["adler"][i] == zlib.adler32(s), i
            if i < 16 or i % oracle_every == 0:
                exp, bits, ocnt = oracle_block(fc, window + s, W, table)
                assert k == len(exp) and r["tebc"][i] == bits % 8 and got == exp, (i, len(s), k, len(exp))
                if cnt is not None:
                    assert (cnt[i] == ocnt).all(), i
            # an independent inflate with the WHOLE dictionary
            z = zlib.decompressobj(-15, zdict=dict_bytes) if dict_bytes else zlib.decompressobj(-15)
            assert z.decompress(got) == s and z.eof, i
    finally:
        d.close()


@functools.lru_cache(maxsize=None)
def source_mix(W, n, seed):
    """n + 24 sources of 0 .. 65536 - W bytes: text, JSON-like, random, zeros; the extremes first, a dozen of any size at the end"""
    top = 65536 - W
    rng = np.random.RandomState(seed)
    sizes = [0, 1, 15, 16, 17, top, top - 1, min(top, 4096), top - 15, top - 16, min(top, 31), min(top, 33)]
    sizes += [int(x) for x in rng.randint(0, min(top, 3000) + 1, n)]
    sizes += [int(x) for x in rng.randint(0, top + 1, 12)]
    kinds = ["text", "json", "random", "zeros"]
    return tuple(record(kinds[i % 4], s, seed + i) for i, s in enumerate(sizes))


# A few thousand jobs a case: the LZ77 kernel is one workgroup per CU that draws job after job, so only a batch of many more jobs
# than CUs runs the second and later trips of its job loop (the LDS image loaded over the previous job's, the window from the
# dictionary again).  Every job against the staged layout and against zlib, the extremes and every 16th against the oracle.
JOBS_A_CASE = 2048


@pytest.mark.parametrize("dl", DICT_LENS)
@pytest.mark.parametrize("fc", ["FHT", "DHTGEN", "DHT_COUNT"])
def test_compress_dict_equals_oracle_and_staged_layout(eng, fc, dl):
    code = getattr(pkg, "FC_COMPRESS_" + fc)
    W = min(dl, 32768) & ~15
    check_compress(eng, make_dict(dl), list(source_mix(W, JOBS_A_CASE, 100 + dl % 1000)), code, oracle_every=16)


def test_compress_dict_thousands_of_small_records(eng):
    """the use the feature is for: 4096 records of 512 bytes against one 32 KiB dictionary"""
    dict_bytes = TEXT[:32768]
    rest = TEXT[32768:]
    recs = [rest[(i * 509) % (len(rest) - 512):][:512] for i in range(4096)]
    check_compress(eng, dict_bytes, recs, pkg.FC_COMPRESS_FHT, oracle_every=16)
    check_compress(eng, dict_bytes, recs[:1024], pkg.FC_COMPRESS_DHTGEN_COUNT, oracle_every=16)


def test_compress_dict_either_spelling_of_the_function_code(eng):
    dict_bytes = make_dict(5000)
    d = eng.dict_create(dict_bytes)
    srcs = source_mix(d.deflate_window, 20, 5)
    a = compress_both(eng, d, dict_bytes, srcs, pkg.FC_COMPRESS_FHT)[0]
    b = compress_both(eng, d, dict_bytes, srcs, pkg.FC_COMPRESS_RESUME_FHT)[0]
    assert a[0].tobytes() == b[0].tobytes()
    for i in range(len(srcs)):
        x, k = int(a[3][i]), int(a[0]["tpbc"][i])
        assert a[1][x:x + k].tobytes() == b[1][x:x + k].tobytes()
    d.close()


@pytest.mark.parametrize("fc", ["FHT", "DHTGEN", "DHT_COUNT"])
def test_compress_dict_refuses_what_does_not_fit(eng, fc):
    code = getattr(pkg, "FC_COMPRESS_" + fc)
    table = builtin_table() if fc == "DHT_COUNT" else None
    dht = eng.to_device(_dht_array([table])) if table else None
    for dl in (32768, 1000, 0):
        dict_bytes = make_dict(dl)
        d = eng.dict_create(dict_bytes)
        W = d.deflate_window
        top = 65536 - W
        # good, too long by one, good, a history of its own, far too long, good
        srcs = [record("text", 700, 1), record("text", top + 1, 2), record("json", top, 3), record("text", 900, 4),
                record("zeros", 70000, 5), record("json", 300, 6)]
        hist = np.array([0, 0, 0, 16, 0, 0], np.uint32)
        bad = [1, 3, 4]
        caps = [int(eng.L.nxz_compress_bound(len(s))) + 512 for s in srcs]
        st, saddr = place(eng, srcs)
        dt, dat = targets(eng, caps, sentinel=0x5b)
        jobs = make_jobs(eng, saddr, [len(s) for s in srcs], dt, dat, caps, hist_len=hist)
        res, _ = eng.compress_dict(code, d, jobs, len(srcs), dht=dht, ntables=1 if table else 0)
        r = eng.results_to_host(res)
        out = dt.cpu().numpy()
        window = dict_bytes[len(dict_bytes) - W:]
        for i, s in enumerate(srcs):
            a = int(dat[i])
            if i in bad:
                assert r["cc"][i] == CC_INVALID_OP and r["tpbc"][i] == 0, (dl, i, r[i])
                assert (out[a:a + ((caps[i] + 31) & ~15)] == 0x5b).all(), (dl, i)
            else:
                exp, bits, _ = oracle_block(code, window + s, W, table)
                k = int(r["tpbc"][i])
                assert r["cc"][i] in (0, 64) and k == len(exp) and out[a:a + k].tobytes() == exp, (dl, i, r[i])
        d.close()


# ---- decompress ---------------------------------------------------------------------------------------------------------
def zraw(data, zdict, level):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 8, zlib.Z_DEFAULT_STRATEGY, zdict) if zdict else zlib.compressobj(level, zlib.DEFLATED, -15)
    return c.compress(data) + c.flush()


def check_against_oracle(r, out, dat, i, stream, cap, window):
    """the verdict of the CPU oracle on the stream with hist = window (tests/test_gpu_parity.py's reading of it)"""
    exp, st = O.inflate(stream, cap, hist=window)
    if st.err:
        assert r["cc"][i] == st.err, (i, r[i], st.err)
    else:
        assert r["cc"][i] in (0, 3), (i, r[i])
        assert r["tpbc"][i] == st.tpbc and out[int(dat[i]):int(dat[i]) + st.tpbc].tobytes() == exp, (i, r[i], st.tpbc)
        assert bool(r["sfbt"][i] & 0x100) == bool(st.final_eob), (i, r[i])
    return st


def decompress_both(eng, d, window, streams, caps, reserved=None, offs=None):
    """the streams through decompress_dict and, staged as [inflate window][stream] with hist_len, through decompress"""
    n = len(streams)
    reserved = reserved if reserved is not None else [0] * n
    lens = np.array([len(s) for s in streams], np.uint32)
    st, saddr = place(eng, streams, offs)
    dt, dat = targets(eng, caps)
    res = eng.decompress_dict(d, make_jobs(eng, saddr, lens, dt, dat, caps, reserved=np.array(reserved, np.uint32)), n)
    r = eng.results_to_host(res).copy()
    reasons = eng.wg_reasons()
    out = dt.cpu().numpy()
    wins = [b"" if f & pkg.JOB_NO_DICT else window for f in reserved]
    st2, saddr2 = place(eng, [w + s for w, s in zip(wins, streams)])
    dt2, dat2 = targets(eng, caps)
    h = np.array([len(w) for w in wins], np.uint32)
    res2 = eng.decompress(make_jobs(eng, saddr2, lens + h, dt2, dat2, caps, hist_len=h,
                                    reserved=np.array([f & 1 for f in reserved], np.uint32)), n)
    r2 = eng.results_to_host(res2).copy()
    out2 = dt2.cpu().numpy()
    return (r, out, dat), (r2, out2, dat2), reasons, h


def assert_same_as_staged(r, out, dat, r2, out2, dat2, h, i):
    for f in ("cc", "tpbc", "tebc", "crc", "adler", "subc", "sfbt"):
        assert r[f][i] == r2[f][i], (i, f, r[i], r2[i])
    assert int(r["spbc"][i]) + int(h[i]) == int(r2["spbc"][i]), (i, r[i], r2[i], h[i])
    k = int(r["tpbc"][i])
    assert out[int(dat[i]):int(dat[i]) + k].tobytes() == out2[int(dat2[i]):int(dat2[i]) + k].tobytes(), i


@pytest.mark.parametrize("dl", [1, 17, 4099, 32768, 50000, 0])
def test_decompress_dict_zlib_and_own_streams(eng, dl, route):
    dict_bytes = make_dict(dl)
    d = eng.dict_create(dict_bytes)
    window = dict_bytes[len(dict_bytes) - d.inflate_window:]
    sizes = [1, 2, 100, 512, 2048, 8192, 40000, 65536, 100000, 300000, 2 << 20]
    plains, streams = [], []
    for i, n in enumerate(sizes * 2):
        p = record(["text", "json", "random", "zeros", "lz"][i % 5], n, 40 + i) if i % 7 else (dict_bytes * (n // max(dl, 1) + 1))[:n] if dl else record("text", n, i)
        plains.append(p)
        streams.append(zraw(p, dict_bytes, [1, 6, 9][i % 3]))
    if dl:
        plains.append(dict_bytes)                      # the dictionary itself: matches that span the whole window
        streams.append(zraw(dict_bytes, dict_bytes, 9))
    # streams of compress_dict itself (sources within 65536 - W)
    W = d.deflate_window
    own = [record(["text", "json", "zeros"][i % 3], s, 90 + i) for i, s in enumerate([0, 1, 300, 512, 5000, 65536 - W])]
    (cr, cout, _, cdat), _, _ = compress_both(eng, d, dict_bytes, own, pkg.FC_COMPRESS_DHTGEN)
    for i, p in enumerate(own):
        plains.append(p)
        streams.append(cout[int(cdat[i]):int(cdat[i]) + int(cr["tpbc"][i])].tobytes())
    caps = [len(p) + (16 if i % 2 else 0) for i, p in enumerate(plains)]
    (r, out, dat), (r2, out2, dat2), reasons, h = decompress_both(eng, d, window, streams, caps)
    assert reasons is not None and reasons["handed_back"] == 0, reasons     # good streams, aligned targets: the workgroup kernel's own
    for i, p in enumerate(plains):
        a = int(dat[i])
        assert r["cc"][i] == CC_OK and r["tpbc"][i] == len(p), (i, r[i])
        assert out[a:a + len(p)].tobytes() == p, i
        assert r["spbc"][i] == len(streams[i]) and r["sfbt"][i] == 0x100 and r["subc"][i] < 8, (i, r[i])
        assert r["crc"][i] == zlib.crc32(p) and r["adler"][i] == zlib.adler32(p), i
        assert (out[a + len(p):a + ((caps[i] + 31) & ~15)] == 0xcd).all(), i          # nothing behind the output, nothing of the dictionary
        assert_same_as_staged(r, out, dat, r2, out2, dat2, h, i)
    d.close()


def test_decompress_dict_thousands_of_mixed_streams(eng, route):
    """a batch of many more streams than CUs: every workgroup takes stream after stream (a stream with the window, then one that
    says NXZ_JOB_NO_DICT, ...), the jobs go ordered by length, and targets that are not 16-byte aligned take the wavefront route
    with the dictionary behind them"""
    dict_bytes = make_dict(32768)
    d = eng.dict_create(dict_bytes)
    rng = np.random.RandomState(11)
    n = 3000
    sizes = [int(x) for x in rng.randint(1, 3000, n - 800)] + [int(x) for x in rng.randint(20000, 120000, 800)]
    rng.shuffle(sizes)
    plains, streams, flags, doffs = [], [], [], []
    for i, sz in enumerate(sizes):
        p = record(["text", "json", "text", "zeros"][i % 4], sz, 500 + i) if i % 11 else dict_bytes[-min(sz, 32768):]
        nodict = i % 5 == 3
        plains.append(p)
        streams.append(zraw(p, b"" if nodict else dict_bytes, [1, 6, 9][i % 3]))
        flags.append(pkg.JOB_NO_DICT if nodict else 0)
        doffs.append(1 + i % 15 if i % 7 == 2 else 0)
    lens = np.array([len(s) for s in streams], np.uint32)
    caps = [len(p) for p in plains]
    st, saddr = place(eng, streams)
    dt, dat = targets(eng, caps, offs=doffs)
    res = eng.decompress_dict(d, make_jobs(eng, saddr, lens, dt, dat, caps, reserved=np.array(flags, np.uint32)), n)
    r = eng.results_to_host(res).copy()
    reasons = eng.wg_reasons()
    out = dt.cpu().numpy()
    assert (r["cc"] == 0).all(), np.nonzero(r["cc"])[0][:8]
    assert (r["tpbc"] == np.array(caps, np.uint32)).all() and (r["spbc"] == lens).all() and (r["sfbt"] == 0x100).all()
    for i, p in enumerate(plains):
        a = int(dat[i])
        assert out[a:a + len(p)].tobytes() == p, (i, len(p), flags[i], doffs[i])
        assert not doffs[i] or out[a - 1] == 0xcd, i                                  # (nothing in front of a shifted target)
        assert out[a + len(p)] == 0xcd, i
        assert r["crc"][i] == zlib.crc32(p) and r["adler"][i] == zlib.adler32(p), i
    # the workgroup kernel hands back exactly the streams it is given whose target is not aligned
    src_min = 0 if route == "workgroup" else 4096
    want = sum(1 for i in range(n) if doffs[i] and lens[i] >= src_min)           # (the sources are 16-byte aligned here)
    assert reasons is not None and reasons["handed_back"] == want and reasons.get("job", 0) == want, (reasons, want)
    assert want > 0 and sum(1 for i in range(n) if doffs[i] == 0 and lens[i] >= max(src_min, 1)) > 256
    d.close()


def test_decompress_dict_bad_streams_among_good_ones(eng, route):
    dict_bytes = make_dict(32768)
    d = eng.dict_create(dict_bytes)
    window = dict_bytes
    good = [record("text", n, 3 + n) for n in (512, 3000, 70000)]
    gs = [zraw(p, dict_bytes, 6) for p in good]
    refs = dict_bytes[-4000:]                                    # a record that is all references to the dictionary
    cases = []                                                   # (stream, cap, flags)
    for p, s in zip(good, gs):
        cases.append((s, len(p), 0))
    cases.append((zraw(refs, dict_bytes, 6), len(refs), pkg.JOB_NO_DICT))          # a distance in front of the (empty) window
    cases.append((gs[1][:len(gs[1]) // 2], len(good[1]), 0))                       # cut short
    dmg = bytearray(gs[2])
    for k in range(300, len(dmg), 97):
        dmg[k] ^= 0x5a
    cases.append((bytes(dmg), len(good[2]), 0))                                    # damaged
    cases.append((gs[1], len(good[1]) - 1, 0))                                     # target too small
    cases.append((gs[2], 20000, pkg.JOB_SUSPEND_WHEN_FULL))                        # ... and a place to suspend
    cases.append((gs[0] + b"\0" * 9, len(good[0]), 0))                             # bytes behind the final block
    cases.append((b"", 100, 0))                                                    # no source at all
    for p, s in zip(good, gs):
        cases.append((s, len(p), 0))
    streams, caps, flags = [c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases]
    (r, out, dat), (r2, out2, dat2), reasons, h = decompress_both(eng, d, window, streams, caps, reserved=flags)
    for i in range(len(cases)):
        assert_same_as_staged(r, out, dat, r2, out2, dat2, h, i)
        if not flags[i] & pkg.JOB_SUSPEND_WHEN_FULL:         # (the oracle has no such flag: that job against the staged layout alone)
            check_against_oracle(r, out, dat, i, streams[i], caps[i], b"" if flags[i] & pkg.JOB_NO_DICT else window)
    assert r["cc"][3] == CC_INVALID_DIST and r["cc"][6] == CC_TARGET_SPACE and r["cc"][7] == CC_DATA_LENGTH and r["tpbc"][7] > 0
    for k, p in enumerate(good):
        for i in (k, len(cases) - 3 + k):
            assert r["cc"][i] == 0 and out[int(dat[i]):int(dat[i]) + len(p)].tobytes() == p, i
    d.close()


def test_decompress_dict_window_shorter_than_the_streams_dictionary(eng, route):
    """a stream made with 32 KiB of dictionary, decoded with its last 1 KiB only"""
    full = make_dict(32768)
    d = eng.dict_create(full[-1024:])
    near, far = full[-900:-100], full[2000:6000]                 # one record refers to the last KiB, one far in front of it
    streams = [zraw(near, full, 9), zraw(far, full, 9), zraw(near, full, 9)]
    caps = [len(near), len(far), len(near)]
    (r, out, dat), (r2, out2, dat2), reasons, h = decompress_both(eng, d, full[-1024:], streams, caps)
    for i, p in enumerate([near, far, near]):
        check_against_oracle(r, out, dat, i, streams[i], caps[i], full[-1024:])
        assert_same_as_staged(r, out, dat, r2, out2, dat2, h, i)
    assert r["cc"][0] == 0 and r["cc"][2] == 0 and out[int(dat[0]):int(dat[0]) + len(near)].tobytes() == near
    assert r["cc"][1] == CC_INVALID_DIST
    d.close()


def test_decompress_dict_refuses_resume_and_history(eng, route):
    dict_bytes = make_dict(4099)
    d = eng.dict_create(dict_bytes)
    p = record("text", 2000, 9)
    s = zraw(p, dict_bytes, 6)
    st, saddr = place(eng, [s, s, s, s])
    dt, dat = targets(eng, [2000] * 4, sentinel=0x77)
    j = np.zeros(4, pkg.JOB_DTYPE)
    j["src"], j["dst"], j["src_len"], j["dst_cap"], j["in_adler"] = saddr, np.uint64(dt.data_ptr()) + dat.astype(np.uint64), len(s), 2000, 1
    j["hist_len"][1] = 16
    j["resume"][2] = 1 << 20
    r = eng.results_to_host(eng.decompress_dict(d, eng.to_device(j), 4))
    out = dt.cpu().numpy()
    for i in (0, 3):
        assert r["cc"][i] == 0 and out[int(dat[i]):int(dat[i]) + 2000].tobytes() == p, (i, r[i])
    for i in (1, 2):
        assert r["cc"][i] == CC_INVALID_OP and r["tpbc"][i] == 0, (i, r[i])
        assert (out[int(dat[i]):int(dat[i]) + 2016] == 0x77).all(), i
    d.close()


# ---- zlib framing -------------------------------------------------------------------------------------------------------
def test_framed_round_trip_and_mixed_batch(eng, route):
    import torch
    dict_bytes = make_dict(32768)
    d = eng.dict_create(dict_bytes)
    W = d.deflate_window
    srcs = [record(["text", "json", "random", "zeros"][i % 4], s, 60 + i) for i, s in enumerate([0, 1, 100, 512, 2048, 8192, 65536 - W, 3000])]
    n = len(srcs)
    caps = [int(eng.L.nxz_compress_bound(len(s))) + 512 for s in srcs]
    st, saddr = place(eng, srcs)
    dt, dat = targets(eng, caps)
    for level, fc in ((6, pkg.FC_COMPRESS_DHTGEN), (1, pkg.FC_COMPRESS_FHT)):
        jobs = make_jobs(eng, saddr, [len(s) for s in srcs], dt, dat, caps)
        res, _ = eng.compress_dict(fc, d, jobs, n)
        packed = torch.zeros(n * 10 + sum(max(c, len(s) + 5) for c, s in zip(caps, srcs)) + 16, dtype=torch.uint8, device=eng.dev)
        offs = eng.pack_zlib_dict(level, d, jobs, res, n, packed)
        torch.cuda.synchronize()
        o = offs.cpu().numpy()
        img = packed.cpu().numpy().tobytes()
        members = [img[o[i]:o[i + 1]] for i in range(n)]
        want_hdr = zlib.compressobj(level, zlib.DEFLATED, 15, 8, zlib.Z_DEFAULT_STRATEGY, dict_bytes).compress(b"x")[:6] or None
        for i, m in enumerate(members):
            assert m[:2] == {6: b"\x78\xbb", 1: b"\x78\x3f"}[level] and m[2:6] == struct.pack(">I", zlib.adler32(dict_bytes)), i
            if want_hdr:
                assert m[:6] == want_hdr
            z = zlib.decompressobj(zdict=dict_bytes)
            assert z.decompress(m) == srcs[i] and z.eof and not z.unused_data, i
        # ... and back through the device
        mt, maddr = place(eng, members, [i % 16 for i in range(n)])
        bt, bat = targets(eng, [len(s) for s in srcs])
        fj = make_jobs(eng, maddr, [len(m) for m in members], bt, bat, [len(s) for s in srcs])
        fr_res, fr = eng.decompress_framed_dict(pkg.FMT_ZLIB, d, fj, n)
        r, f = eng.results_to_host(fr_res), eng.frames_to_host(fr)
        back = bt.cpu().numpy()
        for i, s in enumerate(srcs):
            assert f["status"][i] == pkg.FRAME_OK and f["hdr_len"][i] == 6 and f["dictid"][i] == d.id and f["end"][i] == len(members[i]), (i, f[i])
            assert r["cc"][i] == 0 and r["tpbc"][i] == len(s) and back[int(bat[i]):int(bat[i]) + len(s)].tobytes() == s, (i, r[i])
            assert f["check"][i] == zlib.adler32(s)

    # a mixed batch: FDICT with this id, FDICT with another, plain zlib, gzip, and a cheat
    p = [record("text", 3000, 70 + i) for i in range(5)]
    refs = dict_bytes[-3000:]
    zd = zlib.compressobj(6, zlib.DEFLATED, 15, 8, zlib.Z_DEFAULT_STRATEGY, dict_bytes)
    m_match = zd.compress(p[0]) + zd.flush()
    other = make_dict(500)
    zo = zlib.compressobj(6, zlib.DEFLATED, 15, 8, zlib.Z_DEFAULT_STRATEGY, other)
    m_other = zo.compress(p[1]) + zo.flush()
    m_plain = zlib.compress(p[2], 6)
    m_gzip = F.gzip_member(p[3], 6)
    zc = zlib.compressobj(6, zlib.DEFLATED, 15, 8, zlib.Z_DEFAULT_STRATEGY, dict_bytes)
    cheat = zc.compress(refs) + zc.flush()
    flg = cheat[1] & ~0x20 & ~0x1f
    flg |= 31 - ((cheat[0] << 8 | flg) % 31)
    cheat = bytes([cheat[0], flg]) + cheat[6:]                   # FDICT cleared, FCHECK fixed up, DICTID cut out
    assert (cheat[0] << 8 | cheat[1]) % 31 == 0 and not cheat[1] & 0x20
    with pytest.raises(zlib.error):
        zlib.decompress(cheat)
    zc2 = zlib.compressobj(9, zlib.DEFLATED, 15, 8, zlib.Z_DEFAULT_STRATEGY, dict_bytes)
    m_match2 = zc2.compress(refs) + zc2.flush()
    batch = [m_match, m_other, m_plain, m_gzip, cheat, m_match2]
    plain = [p[0], p[1], p[2], p[3], refs, refs]
    mt, maddr = place(eng, batch)
    bt, bat = targets(eng, [len(x) for x in plain], sentinel=0x33)
    fj = make_jobs(eng, maddr, [len(m) for m in batch], bt, bat, [len(x) for x in plain])
    fr_res, fr = eng.decompress_framed_dict(pkg.FMT_AUTO, d, fj, len(batch))
    r, f = eng.results_to_host(fr_res), eng.frames_to_host(fr)
    back = bt.cpu().numpy()
    got = lambda i: back[int(bat[i]):int(bat[i]) + len(plain[i])].tobytes()
    for i in (0, 2, 3, 5):
        assert f["status"][i] == pkg.FRAME_OK and r["cc"][i] == 0 and got(i) == plain[i], (i, f[i], r[i])
    assert f["hdr_len"][0] == 6 and f["dictid"][0] == d.id and f["hdr_len"][2] == 2 and f["format"][3] == pkg.FMT_GZIP
    assert f["status"][1] == pkg.FRAME_NEED_DICT and f["dictid"][1] == zlib.adler32(other) and r["cc"][1] == CC_INVALID_OP
    assert (back[int(bat[1]):int(bat[1]) + len(plain[1])] == 0x33).all()
    assert f["status"][4] == pkg.FRAME_DEFLATE and r["cc"][4] == CC_INVALID_DIST, (f[4], r[4])
    # the plain framed call still refuses every FDICT stream
    bt2, bat2 = targets(eng, [len(x) for x in plain], sentinel=0x33)
    fj2 = make_jobs(eng, maddr, [len(m) for m in batch], bt2, bat2, [len(x) for x in plain])
    f2 = eng.frames_to_host(eng.decompress_framed(pkg.FMT_AUTO, fj2, len(batch))[1])
    assert [int(x) for x in f2["status"]] == [pkg.FRAME_NEED_DICT, pkg.FRAME_NEED_DICT, pkg.FRAME_OK, pkg.FRAME_OK, pkg.FRAME_DEFLATE, pkg.FRAME_NEED_DICT]
    d.close()


def test_pack_zlib_dict_header_for_every_level(eng):
    import torch
    dict_bytes = make_dict(777)
    d = eng.dict_create(dict_bytes)
    s = record("text", 1000, 1)
    st, saddr = place(eng, [s])
    cap = int(eng.L.nxz_compress_bound(len(s))) + 512           # (+ 512: a dynamic block's table)
    dt, dat = targets(eng, [cap])
    jobs = make_jobs(eng, saddr, [len(s)], dt, dat, [cap])
    res, _ = eng.compress_dict(pkg.FC_COMPRESS_FHT, d, jobs, 1)
    for level in range(-1, 10):
        packed = torch.zeros(cap + 32, dtype=torch.uint8, device=eng.dev)
        offs = eng.pack_zlib_dict(level, d, jobs, res, 1, packed)
        torch.cuda.synchronize()
        m = packed.cpu().numpy().tobytes()[:int(offs.cpu().numpy()[1])]
        zc = zlib.compressobj(level, zlib.DEFLATED, 15, 8, zlib.Z_DEFAULT_STRATEGY, dict_bytes)
        want = zc.compress(s) + zc.flush()
        assert m[:6] == want[:6], (level, m[:6].hex(), want[:6].hex())
        assert zlib.decompressobj(zdict=dict_bytes).decompress(m) == s
    d.close()


# ---- an empty dictionary: the plain calls, byte for byte ------------------------------------------------------------------
def test_empty_dictionary_equals_the_plain_calls(eng):
    import torch
    d = eng.dict_create(b"")
    assert d.id == 1 and d.inflate_window == 0 and d.deflate_window == 0
    srcs = [record(["text", "json", "random", "zeros"][i % 4], s, 80 + i) for i, s in enumerate([0, 1, 17, 512, 5000, 65536])]
    n = len(srcs)
    for fc in (pkg.FC_COMPRESS_FHT, pkg.FC_COMPRESS_DHTGEN_COUNT):
        (r, out, cnt, dat), (r2, out2, cnt2, _), _ = compress_both(eng, d, b"", srcs, fc)
        assert r.tobytes() == r2.tobytes()
        assert cnt is None or (cnt == cnt2).all()
        for i in range(n):
            a, k = int(dat[i]), int(r["tpbc"][i])
            assert out[a:a + k].tobytes() == out2[a:a + k].tobytes(), i
    streams = [zlib.compress(s, 6)[2:-4] for s in srcs]
    caps = [len(s) for s in srcs]
    (r, out, dat), (r2, out2, dat2), reasons, h = decompress_both(eng, d, b"", streams, caps)
    assert r.tobytes() == r2.tobytes() and out.tobytes() == out2.tobytes()
    # pack: the plain members with FDICT and DICTID 1 in the header
    ccaps = [int(eng.L.nxz_compress_bound(len(s))) + 512 for s in srcs]
    st, saddr = place(eng, srcs)
    dt, dat = targets(eng, ccaps)
    jobs = make_jobs(eng, saddr, [len(s) for s in srcs], dt, dat, ccaps)
    res, _ = eng.compress_dict(pkg.FC_COMPRESS_FHT, d, jobs, n)
    room = n * 10 + sum(max(c, len(s) + 5) for c, s in zip(ccaps, srcs)) + 16
    pa, pb = torch.zeros(room, dtype=torch.uint8, device=eng.dev), torch.zeros(room, dtype=torch.uint8, device=eng.dev)
    oa = eng.pack_zlib_dict(6, d, jobs, res, n, pa)
    ob = eng.pack_zlib(6, jobs, res, n, pb)
    torch.cuda.synchronize()
    oa, ob, ia, ib = oa.cpu().numpy(), ob.cpu().numpy(), pa.cpu().numpy().tobytes(), pb.cpu().numpy().tobytes()
    members = []
    for i in range(n):
        ma, mb = ia[oa[i]:oa[i + 1]], ib[ob[i]:ob[i + 1]]
        assert ma[:6] == b"\x78\xbb\0\0\0\1" and ma[6:] == mb[2:], i
        assert zlib.decompressobj(zdict=b"").decompress(ma) == srcs[i], i
        members.append((ma, mb))
    # framed: FDICT with DICTID 1 is this dictionary's; plain streams as the plain call reads them
    batch = [m[0] for m in members] + [m[1] for m in members]
    mt, maddr = place(eng, batch)
    bt, bat = targets(eng, caps * 2)
    fj = make_jobs(eng, maddr, [len(m) for m in batch], bt, bat, caps * 2)
    fr_res, fr = eng.decompress_framed_dict(pkg.FMT_ZLIB, d, fj, 2 * n)
    r, f = eng.results_to_host(fr_res).copy(), eng.frames_to_host(fr).copy()
    back = bt.cpu().numpy()
    bt2, bat2 = targets(eng, caps * 2)
    fj2 = make_jobs(eng, maddr, [len(m) for m in batch], bt2, bat2, caps * 2)
    fr_res2, fr2 = eng.decompress_framed(pkg.FMT_ZLIB, fj2, 2 * n)
    r2, f2 = eng.results_to_host(fr_res2), eng.frames_to_host(fr2)
    for i in range(2 * n):
        s = srcs[i % n]
        assert f["status"][i] == pkg.FRAME_OK and r["cc"][i] == 0 and back[int(bat[i]):int(bat[i]) + len(s)].tobytes() == s, (i, f[i], r[i])
        if i >= n:
            assert r[i].tobytes() == r2[i].tobytes() and f[i].tobytes() == f2[i].tobytes(), i
        else:
            assert f2["status"][i] == pkg.FRAME_NEED_DICT
    d.close()
