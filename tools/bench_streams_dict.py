"""nxz_batch_deflate_streams_dict (zlib, exact table per block, hist_max 32768) beside what the batched API had before it.
(a) 65 536 JSON-like records of 256 B to 4 KiB and one 32 KiB dictionary of such rows: the rate against nxz_batch_compress_dict +
    nxz_batch_pack_zlib_dict on the same records (the route for sources that fit a block), the compressed bytes against
    nxz_batch_deflate_streams, which has no dictionary;
(b) 4096 streams of 1 MiB of the corpus bytes, tiled: the rate against nxz_batch_deflate_streams at the same hist_max (the
    dictionary call adds two small launches a chunk: the first blocks' LZ77 launch and the gather).
Each call is warmed up once and timed REPS times with device events; the rate is source GiB/s over the median.
usage: bench_streams_dict.py [out.txt] -> profiles/r19_streams_dict.txt.  RECORDS / STREAMS pick other counts."""
import importlib, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import corpus
pkg = importlib.import_module("power-gzip_amd")
E = pkg.engine
REPS = int(os.environ.get("REPS", "5"))
RECORDS, STREAMS = int(os.environ.get("RECORDS", "65536")), int(os.environ.get("STREAMS", "4096"))
HIST, FC = 32768, pkg.FC_COMPRESS_DHTGEN
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def timed(f):
    f()
    torch.cuda.synchronize()
    ms = []
    for _ in range(REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        f()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), min(ms), max(ms)


def rows(n, first):
    out, i = [], first
    while sum(map(len, out)) < n:
        out.append(b'{"id": %d, "name": "user%d", "active": %s, "tags": ["a%d", "b"], "score": %d.%d}\n'
                   % (i, i % 97, b"true" if i % 3 else b"false", i % 7, i * 31 % 1000, i % 10))
        i += 1
    return b"".join(out)[:n]


def streams_call(d, src, lens, stride):
    """one stream per buffer, with the Dict d or (None) without"""
    n = len(lens)
    bound = eng.deflate_stream_bound_dict if d is not None else eng.deflate_stream_bound
    caps = np.array([bound(int(x), HIST, E.FMT_ZLIB) for x in np.unique(lens)], np.uint64)[np.searchsorted(np.unique(lens), lens)]
    at = np.concatenate([[0], np.cumsum((caps + np.uint64(15)) & ~np.uint64(15))]).astype(np.uint64)
    dst = torch.empty(int(at[-1]), dtype=torch.uint8, device=eng.dev)
    j = np.zeros(n, E.STREAM_JOB_DTYPE)
    j["src"] = np.uint64(src.data_ptr()) + np.arange(n, dtype=np.uint64) * np.uint64(stride)
    j["dst"], j["src_len"], j["dst_cap"] = np.uint64(dst.data_ptr()) + at[:-1], lens, caps
    res = torch.empty(n * E.STREAM_RESULT_DTYPE.itemsize, dtype=torch.uint8, device=eng.dev)

    def f():
        if d is not None:
            rc, _ = eng.deflate_stream_jobs_dict(FC, E.FMT_ZLIB, d, j, results=res, hist_max=HIST)
        else:
            rc, _ = eng.deflate_stream_jobs(FC, E.FMT_ZLIB, j, results=res, hist_max=HIST)
        assert rc == 0, rc
    t = timed(f)
    r = eng.results_to_host(res, E.STREAM_RESULT_DTYPE)
    assert (r["cc"] == 0).all()
    return t, int(r["out_len"].sum())


def per_record_call(d, src, lens, stride):
    """a job per record: nxz_batch_compress_dict, then nxz_batch_pack_zlib_dict"""
    n, S = len(lens), 8192
    out = torch.empty((n, S), dtype=torch.uint8, device=eng.dev)
    jobs = eng.jobs_strided(src, stride, lens.astype(np.uint32), out, S, S)
    res = torch.empty(n * E.RESULT_DTYPE.itemsize, dtype=torch.uint8, device=eng.dev)
    packed = torch.empty(n * (stride + 32), dtype=torch.uint8, device=eng.dev)
    offs = torch.empty(n + 1, dtype=torch.int64, device=eng.dev)

    def f():
        eng.compress_dict(FC, d, jobs, n, results=res)
        eng.pack_zlib_dict(-1, d, jobs, res, n, packed, offsets=offs)
    t = timed(f)
    torch.cuda.synchronize()
    return t, int(offs[-1].item())


def gibs(total, ms):
    return total / ms / 1e-3 / 2 ** 30


eng = pkg.Engine(0)
dict_bytes = rows(32768, 7000)
d = eng.dict_create(dict_bytes)

# (a) records
stride = 4096
rnd = np.random.default_rng(19)
lens = rnd.integers(256, 4097, RECORDS)
pool = np.frombuffer(rows(8 << 20, 100000), np.uint8)
starts = rnd.integers(0, len(pool) - stride, RECORDS)
host = pool[starts[:, None] + np.arange(stride)[None, :]]
src = torch.from_numpy(np.ascontiguousarray(host)).to(eng.dev)
total = int(lens.sum())
(dm, dlo, dhi), dbytes = streams_call(d, src, lens, stride)
(pm, plo, phi), pbytes = per_record_call(d, src, lens, stride)
(nm, nlo, nhi), nbytes = streams_call(None, src, lens, stride)
say("(a) %d records of 256 B to 4 KiB (%.1f MiB), one 32 KiB dictionary, zlib, DHTGEN, hist_max %d" % (RECORDS, total / 2 ** 20, HIST))
say("  deflate_streams_dict            %7.2f GiB/s  ratio %6.3f  %11d bytes   (%.2f ms, %.2f..%.2f)" % (gibs(total, dm), total / dbytes, dbytes, dm, dlo, dhi))
say("  compress_dict + pack_zlib_dict  %7.2f GiB/s  ratio %6.3f  %11d bytes   (%.2f ms, %.2f..%.2f)" % (gibs(total, pm), total / pbytes, pbytes, pm, plo, phi))
say("  deflate_streams (no dictionary) %7.2f GiB/s  ratio %6.3f  %11d bytes   (%.2f ms, %.2f..%.2f)" % (gibs(total, nm), total / nbytes, nbytes, nm, nlo, nhi))
say("  rate against the per-record route: %.2f; compressed bytes against the call without a dictionary: %.3f" % (pm / dm, dbytes / nbytes))
del src, host
torch.cuda.empty_cache()

# (b) long streams
B = 65536
_, blocks, _ = corpus.load(B)
unit = torch.from_numpy(np.frombuffer(b"".join(b for _, _, b in blocks if len(b) == B), np.uint8).copy()).to(eng.dev)
size = 1 << 20
total = STREAMS * size
src = unit.repeat(-(-total // unit.numel()))[:total].contiguous()
lens = np.full(STREAMS, size, np.int64)
(dm, dlo, dhi), dbytes = streams_call(d, src, lens, size)
(nm, nlo, nhi), nbytes = streams_call(None, src, lens, size)
say("(b) %d streams of 1 MiB, zlib, DHTGEN, hist_max %d" % (STREAMS, HIST))
say("  deflate_streams_dict            %7.2f GiB/s  ratio %6.3f   (%.1f ms, %.1f..%.1f)" % (gibs(total, dm), total / dbytes, dm, dlo, dhi))
say("  deflate_streams                 %7.2f GiB/s  ratio %6.3f   (%.1f ms, %.1f..%.1f)" % (gibs(total, nm), total / nbytes, nm, nlo, nhi))
say("  rate against the plain call: %.3f" % (nm / dm))
d.close()
eng.close()
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        f.write("\n".join(lines) + "\n")
