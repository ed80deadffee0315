"""nxz_batch_deflate_streams_part (zlib, exact table per block) beside nxz_batch_deflate_streams on the same bytes:
(a) the plain call: every stream of 1 MiB in one call;
(p1) the part call with every stream as ONE part (FIRST | LAST): the same compress kernels, so what differs is the part's own
     prologue / expand / layout / pack / epilogue -- it should sit inside (a)'s own run-to-run spread;
(c4, c16) every stream written in 4 parts of 256 KiB / 16 parts of 64 KiB, a call a part, the parts one behind the other in memory
     (prev + prev_len == src: nothing is staged);
(d4, d16) the same with prev detached -- a copy of the last 32 KiB in front of the part, elsewhere and at an odd address -- so that
     every part's first block goes through the staging kernel.
The corpus bytes, tiled, as 4096 streams of 1 MiB; hist_max 0 and 32768.  Each route is warmed up once, then all are timed in turn
REPS times (a host clock around work that ends in a device synchronise; the calls of a route are queued back to back, the carry goes
from call to call on the device) and the medians are compared.  (c) and (d) against (a) show what the per-call fixed phases and
the staging cost; with hist_max 0 no block has a window and (d) is (c).
usage: bench_streams_part.py [out.txt] -> profiles/r24_streams_part.txt.  SHAPE=streams x KiB picks another shape (the default
needs about 14 GiB of device memory)."""
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
N, KIB = (int(v) for v in os.environ.get("SHAPE", "4096x1024").split("x"))
SPLITS = [int(x) for x in os.environ.get("SPLITS", "4,16").split(",")]
FC, FMT = pkg.FC_COMPRESS_DHTGEN, E.FMT_ZLIB
KEEP = 32768
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
size, total = KIB * 1024, N * KIB * 1024
src = unit.repeat(-(-total // unit.numel()))[:total].contiguous()
idx = np.arange(N, dtype=np.uint64)


def point(hist_max):
    t = torch
    bound = eng.deflate_stream_bound(size, hist_max, FMT)
    stride = (bound + 15 + 32 * 16) & ~15                      # room for every part's own end: 16 parts, a few bytes each
    dst = {k: t.empty(N * stride, dtype=t.uint8, device=eng.dev) for k in ("a", "p")}
    res = t.empty(N * E.STREAM_RESULT_DTYPE.itemsize, dtype=t.uint8, device=eng.dev)
    carry = t.zeros(N * E.STREAM_CARRY_DTYPE.itemsize, dtype=t.uint8, device=eng.dev)
    ja = np.zeros(N, E.STREAM_JOB_DTYPE)
    ja["src"], ja["dst"] = np.uint64(src.data_ptr()) + idx * np.uint64(size), np.uint64(dst["a"].data_ptr()) + idx * np.uint64(stride)
    ja["src_len"], ja["dst_cap"] = size, bound
    # the detached windows: the KEEP bytes in front of every part but a stream's first, copied elsewhere, one byte off a 16-byte boundary
    wstride = KEEP + 16

    def part_jobs(parts, detached):
        plen, jobs = size // parts, []
        win = t.empty(N * parts * wstride + 16, dtype=t.uint8, device=eng.dev) if detached else None
        for k in range(parts):
            j = np.zeros(N, E.STREAM_PART_JOB_DTYPE)
            j["src"] = np.uint64(src.data_ptr()) + idx * np.uint64(size) + np.uint64(k * plen)
            # every part has the room of its bound: the parts of a stream go one behind the other at these strides
            pb = eng.deflate_stream_part_bound(plen, hist_max, FMT, (E.PART_FIRST if k == 0 else 0) | (E.PART_LAST if k == parts - 1 else 0))
            j["dst"] = np.uint64(dst["p"].data_ptr()) + idx * np.uint64(stride) + np.uint64(k * ((stride // parts) & ~15))
            j["src_len"], j["dst_cap"] = plen, (stride // parts) & ~15
            j["flags"] = (E.PART_FIRST if k == 0 else 0) | (E.PART_LAST if k == parts - 1 else 0)
            if k:
                keep = min(KEEP, k * plen)
                if detached:
                    at = (idx * np.uint64(parts) + np.uint64(k)) * np.uint64(wstride) + np.uint64(1)
                    view = src.view(N, size)[:, k * plen - keep:k * plen]
                    win[1:1 + N * parts * wstride].view(N, parts, wstride)[:, k, :keep] = view
                    j["prev"] = np.uint64(win.data_ptr()) + at
                else:
                    j["prev"] = j["src"] - np.uint64(keep)
                j["prev_len"] = keep
            assert (j["dst_cap"] >= pb).all(), "a part's target is smaller than its bound"
            jobs.append(j)
        return jobs, win

    def a():
        rc, _ = eng.deflate_stream_jobs(FC, FMT, ja, results=res, hist_max=hist_max)
        assert rc == 0, rc

    def parts_route(jobs):
        def f():
            for j in jobs:
                rc, _ = eng.deflate_stream_parts(FC, FMT, j, carry, results=res, hist_max=hist_max)
                assert rc == 0, rc
        return f

    routes, keepalive = {"a": a}, []
    pj, _ = part_jobs(1, False)
    routes["p1"] = parts_route(pj)
    for parts in SPLITS:
        for tag, det in (("c", False), ("d", True)):
            jobs, win = part_jobs(parts, det)
            keepalive.append(win)
            routes["%s%d" % (tag, parts)] = parts_route(jobs)
    for f in routes.values():
        clocked(f)
    ms = {k: [] for k in routes}
    for _ in range(REPS):
        for k, f in routes.items():
            ms[k].append(clocked(f))
    # (p1) writes what (a) writes
    clocked(a)
    ra = eng.results_to_host(res, E.STREAM_RESULT_DTYPE)[:N].copy()
    clocked(routes["p1"])
    rp = eng.results_to_host(res, E.STREAM_RESULT_DTYPE)[:N].copy()
    assert ra.tobytes() == rp.tobytes() and (ra["cc"] == 0).all(), "the part call and the plain call disagree about a whole stream"
    live = t.arange(stride, device=eng.dev)[None, :] < t.from_numpy(ra["out_len"].astype(np.int64)).to(eng.dev)[:, None]
    assert not bool(((dst["a"].view(N, stride) != dst["p"].view(N, stride)) & live).any()), "the part call and the plain call write other bytes"
    return {k: (statistics.median(v), min(v), max(v)) for k, v in ms.items()}


say("%d streams of %d KiB, zlib, DHTGEN; ms per route: median (min..max) of %d, and the ratio to (a)" % (N, KIB, REPS))
for hist_max in (0, 32768):
    m = point(hist_max)
    am = m["a"][0]
    say("hist_max %5d  (a) plain call            %8.2f (%.2f..%.2f)  %6.1f GiB/s" % (hist_max, am, m["a"][1], m["a"][2], total / am / 1e-3 / 2 ** 30))
    names = {"p1": "one part, FIRST | LAST"}
    for parts in SPLITS:
        names["c%d" % parts] = "%d parts of %d KiB, contiguous" % (parts, KIB // parts)
        names["d%d" % parts] = "%d parts of %d KiB, detached" % (parts, KIB // parts)
    for k, name in names.items():
        med, lo, hi = m[k]
        say("hist_max %5d  (%s) %-28s %8.2f (%.2f..%.2f)  %6.1f GiB/s  %.3f of (a)" % (hist_max, k, name, med, lo, hi, total / med / 1e-3 / 2 ** 30, med / am))
    torch.cuda.empty_cache()
eng.close()
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        f.write("\n".join(lines) + "\n")
