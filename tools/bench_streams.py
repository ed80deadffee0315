"""nxz_batch_deflate_streams (zlib, exact table per block) beside the closest the batched API had before it: nxz_batch_compress
+ nxz_batch_pack_zlib on the same bytes cut into 64 KiB jobs, a member per block.  The corpus bytes, tiled, as 4096 streams of
1 MiB, 65 536 streams of 64 KiB and one stream of 1 GiB; hist_max 0 and 32768 (the per-block path has no window: its figure is the
same in both rows); then the first shape at NXZ_STREAMS_CHUNK = 1024 / 4096 / 16384.  Each call is warmed up once and timed REPS
times with device events; the rate is source GiB/s over the median.  usage: bench_streams.py [out.txt]
-> profiles/r11_streams.txt.  SHAPES=streams x KiB,... picks other shapes (the defaults need about 20 GiB of device memory)."""
import importlib, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import corpus
pkg = importlib.import_module("power-gzip_amd")
E = pkg.engine
B, S = 65536, 73856
REPS = int(os.environ.get("REPS", "5"))
shapes = [tuple(int(v) for v in x.split("x")) for x in os.environ.get("SHAPES", "4096x1024,65536x64,1x1048576").split(",")]
chunks = [int(x) for x in os.environ.get("CHUNKS", "1024,4096,16384").split(",")]
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


eng = pkg.Engine(0)
_, blocks, _ = corpus.load(B)
unit = torch.from_numpy(np.frombuffer(b"".join(b for _, _, b in blocks if len(b) == B), np.uint8).copy()).to(eng.dev)


def source(total):
    rep = -(-total // unit.numel())
    return unit.repeat(rep)[:total].contiguous()


def streams_call(src, n, size, hist_max):
    bound = eng.deflate_stream_bound(size, hist_max, E.FMT_ZLIB)
    stride = (bound + 15) & ~15
    dst = torch.empty(n * stride, dtype=torch.uint8, device=eng.dev)
    j = np.zeros(n, E.STREAM_JOB_DTYPE)
    idx = np.arange(n, dtype=np.uint64)
    j["src"], j["dst"] = np.uint64(src.data_ptr()) + idx * np.uint64(size), np.uint64(dst.data_ptr()) + idx * np.uint64(stride)
    j["src_len"], j["dst_cap"] = size, bound
    res = torch.empty(n * E.STREAM_RESULT_DTYPE.itemsize, dtype=torch.uint8, device=eng.dev)

    def f():
        rc, _ = eng.deflate_stream_jobs(pkg.FC_COMPRESS_DHTGEN, E.FMT_ZLIB, j, results=res, hist_max=hist_max)
        assert rc == 0, rc
    t = timed(f)
    r = eng.results_to_host(res, E.STREAM_RESULT_DTYPE)
    assert (r["cc"] == 0).all()
    return t, int(r["out_len"].sum())


def per_block_call(src, total):
    nb = total // B
    out = torch.empty((nb, S), dtype=torch.uint8, device=eng.dev)
    jobs = eng.jobs_strided(src, B, np.full(nb, B, np.uint32), out, S, S)
    res = torch.empty(nb * E.RESULT_DTYPE.itemsize, dtype=torch.uint8, device=eng.dev)
    packed = torch.empty(nb * (B + 16), dtype=torch.uint8, device=eng.dev)
    offs = torch.empty(nb + 1, dtype=torch.int64, device=eng.dev)

    def f():
        eng.compress(pkg.FC_COMPRESS_DHTGEN, jobs, nb, results=res)
        eng.pack_zlib(-1, jobs, res, nb, packed, offsets=offs)
    t = timed(f)
    torch.cuda.synchronize()
    return t, int(offs[-1].item())


say("%-22s %9s | %14s %9s | %14s %9s | %6s" % ("shape", "hist_max", "streams GiB/s", "ratio", "per-block GiB/s", "ratio", "s / pb"))
for n, kib in shapes:
    size, total = kib * 1024, n * kib * 1024
    src = source(total)
    (pm, _, _), pbytes = per_block_call(src, total)
    for hist_max in (0, 32768):
        (sm, lo, hi), sbytes = streams_call(src, n, size, hist_max)
        gs, gp = total / sm / 1e-3 / 2 ** 30, total / pm / 1e-3 / 2 ** 30
        say("%-22s %9d | %14.1f %9.3f | %14.1f %9.3f | %6.2f   (%.1f ms, %.1f..%.1f)" % ("%d x %d KiB" % (n, kib), hist_max, gs, total / sbytes, gp,
                                                                                total / pbytes, gs / gp, sm, lo, hi))
    del src
    torch.cuda.empty_cache()
n, kib = shapes[0]
src = source(n * kib * 1024)
say("NXZ_STREAMS_CHUNK, %d x %d KiB, hist_max 0:" % (n, kib))
for c in chunks:
    os.environ["NXZ_STREAMS_CHUNK"] = str(c)
    (sm, lo, hi), _ = streams_call(src, n, kib * 1024, 0)
    say("  %6d blocks a chunk: %7.1f GiB/s   (%.1f ms, %.1f..%.1f)" % (c, n * kib * 1024 / sm / 1e-3 / 2 ** 30, sm, lo, hi))
os.environ.pop("NXZ_STREAMS_CHUNK", None)
eng.close()
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        f.write("\n".join(lines) + "\n")
