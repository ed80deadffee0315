"""nxz_batch_deflate_streams_indexed (zlib, exact table per block) beside the two things it stands between:
(a) nxz_batch_deflate_streams alone -- the streams without an index;
(b) the route to the same index before this call: nxz_batch_deflate_streams, the host wait for every out_len, the index jobs built on
    the host and uploaded, then nxz_batch_checkpoint_index with its windows copied from the source (jobs[i].dst = the source);
(c) the new call: streams, rows and windows in one asynchronous call.
The corpus bytes, tiled, as 4096 streams of 1 MiB and 64 streams of 16 MiB; hist_max 0 and 32768; a checkpoint every 64 KiB and
every 1 MiB.  Each route is warmed up once, then the three are timed in turn REPS times (a host clock around work that ends in a
device synchronise: route (b) has host work in the middle) and the medians are compared.  (c) does a subset of (b)'s work, so
(c) / (b) above 1 at any point means something is wrong; (c) / (a) is what the index costs, its floor the windows' traffic
(32 KiB a stored checkpoint).  The rows of (b) and (c) are compared once per point.
usage: bench_streams_indexed.py [out.txt] -> profiles/r23_streams_indexed.txt.  SHAPES=streams x KiB,... picks other shapes (the
defaults need about 16 GiB of device memory)."""
import importlib, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import corpus
pkg = importlib.import_module("power-gzip_amd")
E = pkg.engine
B = 65536
REPS = int(os.environ.get("REPS", "5"))
shapes = [tuple(int(v) for v in x.split("x")) for x in os.environ.get("SHAPES", "4096x1024,64x16384").split(",")]
spans = [int(x) * 1024 for x in os.environ.get("SPANS_KIB", "64,1024").split(",")]
FC, FMT = pkg.FC_COMPRESS_DHTGEN, E.FMT_ZLIB
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def clocked(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


eng = pkg.Engine(0)
_, blocks, _ = corpus.load(B)
unit = torch.from_numpy(np.frombuffer(b"".join(b for _, _, b in blocks if len(b) == B), np.uint8).copy()).to(eng.dev)


def source(total):
    rep = -(-total // unit.numel())
    return unit.repeat(rep)[:total].contiguous()


def point(src, n, size, hist_max, span):
    t = torch
    bound = eng.deflate_stream_bound(size, hist_max, FMT)
    stride = (bound + 15) & ~15
    dst = t.empty(n * stride, dtype=t.uint8, device=eng.dev)
    j = np.zeros(n, E.STREAM_JOB_DTYPE)
    idx = np.arange(n, dtype=np.uint64)
    j["src"], j["dst"] = np.uint64(src.data_ptr()) + idx * np.uint64(size), np.uint64(dst.data_ptr()) + idx * np.uint64(stride)
    j["src_len"], j["dst_cap"] = size, bound
    res = t.empty(n * E.STREAM_RESULT_DTYPE.itemsize, dtype=t.uint8, device=eng.dev)
    cp_cap = size // span + 2
    rows = {k: (t.zeros((n, cp_cap + 1), dtype=t.int64, device=eng.dev), t.zeros((n, cp_cap + 1), dtype=t.int64, device=eng.dev),
                t.zeros((n, cp_cap, E.CHECKPOINT_WINDOW), dtype=t.uint8, device=eng.dev),
                t.zeros(n * E.CHECKPOINT_STREAM_DTYPE.itemsize, dtype=t.uint8, device=eng.dev)) for k in "bc"}
    ij = t.zeros(n * E.JOB_DTYPE.itemsize, dtype=t.uint8, device=eng.dev)

    def a():
        rc, _ = eng.deflate_stream_jobs(FC, FMT, j, results=res, hist_max=hist_max)
        assert rc == 0, rc

    def b():
        a()
        r = eng.results_to_host(res, E.STREAM_RESULT_DTYPE)             # the host wait for out_len
        q = np.zeros(n, E.JOB_DTYPE)
        q["src"], q["src_len"], q["dst"], q["dst_cap"], q["in_adler"] = j["dst"], r["out_len"], j["src"], size, 1
        cbit, uoff, win, st = rows["b"]
        rc = eng.checkpoint_index(FMT, eng.to_device(q), n, span, cp_cap, windows=win, cbit=cbit, uoff=uoff, streams=st)[0]
        assert rc == 0, rc

    def c():
        cbit, uoff, win, st = rows["c"]
        rc = eng.deflate_stream_jobs_indexed(FC, FMT, j, span, cp_cap, windows=win, index_jobs=ij, results=res, hist_max=hist_max, cbit=cbit, uoff=uoff,
                                             streams=st)[0]
        assert rc == 0, rc

    for f in (a, b, c):
        clocked(f)
    ms = {"a": [], "b": [], "c": []}
    for _ in range(REPS):
        for k, f in (("a", a), ("b", b), ("c", c)):
            ms[k].append(clocked(f))
    # the same index by both routes
    sb, sc = (eng.results_to_host(rows[k][3], E.CHECKPOINT_STREAM_DTYPE)[:n] for k in "bc")
    assert sb.tobytes() == sc.tobytes() and (sc["status"] == pkg.CPS_OK).all(), "the routes disagree about the streams' records"
    live = t.arange(cp_cap + 1, device=eng.dev)[None, :] <= t.from_numpy(sc["count"].astype(np.int64)).to(eng.dev)[:, None]
    assert bool((rows["b"][0][live] == rows["c"][0][live]).all()) and bool((rows["b"][1][live] == rows["c"][1][live]).all()), "the routes disagree about the rows"
    stored = int(sc["count"].sum())
    return {k: (statistics.median(v), min(v), max(v)) for k, v in ms.items()}, stored


say("%-18s %8s %9s | %9s %9s %9s | %7s %7s | %s" % ("shape", "hist_max", "span KiB", "(a) ms", "(b) ms", "(c) ms", "(c)/(a)", "(c)/(b)", "checkpoints, (c) source GiB/s, spreads"))
worst = 0.0
for n, kib in shapes:
    size, total = kib * 1024, n * kib * 1024
    src = source(total)
    for hist_max in (0, 32768):
        for span in spans:
            m, stored = point(src, n, size, hist_max, span)
            (am, alo, ahi), (bm, blo, bhi), (cm, clo, chi) = m["a"], m["b"], m["c"]
            worst = max(worst, cm / bm)
            say("%-18s %8d %9d | %9.2f %9.2f %9.2f | %7.3f %7.3f | %d, %.1f, a %.2f..%.2f b %.2f..%.2f c %.2f..%.2f" % (
                "%d x %d KiB" % (n, kib), hist_max, span // 1024, am, bm, cm, cm / am, cm / bm, stored, total / cm / 1e-3 / 2 ** 30, alo, ahi, blo, bhi, clo, chi))
    del src
    torch.cuda.empty_cache()
say("(c) / (b) at its worst: %.3f -- %s" % (worst, "the new call is slower than the old route nowhere" if worst <= 1.0 else "THE NEW CALL LOSES TO THE OLD ROUTE SOMEWHERE"))
eng.close()
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        f.write("\n".join(lines) + "\n")
sys.exit(0 if worst <= 1.0 else 1)
