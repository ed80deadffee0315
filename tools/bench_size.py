"""The output-size query beside the decode it spares: nxz_batch_decompress_size and nxz_batch_decompress (the engine's own route
for the batch) on the same raw streams in one process, dst_cap of the decode taken from the size results.  Three kinds of
stream -- zlib -6 streams of the corpus blocks, the engine's own exact-table streams of the corpus, its own fixed-code streams of
the synthetic blocks -- at 4096 and 65 536 streams.  Each call is warmed up once, then timed REPS times with device events,
the two calls alternating; the rate is uncompressed GiB/s over the median.  usage: bench_size.py [out.txt]
-> profiles/r10_size.txt"""
import importlib, os, statistics, sys, zlib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import bench, corpus
pkg = importlib.import_module("power-gzip_amd")
B, S = 65536, 73856
REPS = int(os.environ.get("REPS", "7"))
sizes = [int(x) for x in os.environ.get("SIZES", "4096,65536").split(",")]
_, blocks, _ = corpus.load(B)
raw = [b for _, _, b in blocks if len(b) == B]
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def once(f):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    res = f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), res


eng = pkg.Engine(0)
say("%-32s %8s | %12s %12s %8s | %s" % ("streams", "n", "size GiB/s", "decode GiB/s", "ratio", "ms: size / decode (median of %d, min..max)" % REPS))
for kind in ("zlib -6 of the corpus blocks", "own exact tables (corpus)", "own fixed-code (synthetic)"):
    for n in sizes:
        if kind.startswith("zlib"):
            streams = []
            for b in raw:
                c = zlib.compressobj(6, zlib.DEFLATED, -15)
                streams.append(c.compress(b) + c.flush())
            cs = (max(len(s) for s in streams) + 64 + 15) & ~15
            host = np.zeros((len(raw), cs), np.uint8)
            for i, s in enumerate(streams):
                host[i, :len(s)] = np.frombuffer(s, np.uint8)
            rep = -(-n // len(raw))
            src = torch.from_numpy(host).to(eng.dev).repeat(rep, 1)[:n].contiguous()
            clen = np.tile(np.array([len(s) for s in streams], np.uint32), rep)[:n]
        else:
            if "synthetic" in kind:
                data, fc = bench.gen_blocks(torch, eng.dev, n, 0), pkg.FC_COMPRESS_FHT
            else:
                data = torch.from_numpy(np.stack([np.frombuffer(raw[i % len(raw)], np.uint8) for i in range(n)])).to(eng.dev)
                fc = pkg.FC_COMPRESS_DHTGEN
            src = torch.empty((n, S), dtype=torch.uint8, device=eng.dev)
            j1 = eng.jobs_strided(data, B, np.full(n, B, np.uint32), src, S, S)
            clen = eng.results_to_host(eng.compress(fc, j1, n)[0])["tpbc"].astype(np.uint32)
            cs = S
            del data
        dst = torch.zeros((n, B), dtype=torch.uint8, device=eng.dev)
        jobs_size = eng.jobs_strided(src, cs, clen, dst, B, 0xffffffff)
        sized = eng.results_to_host(eng.decompress_size(jobs_size, n))
        assert (sized["cc"] == 0).all() and (sized["tpbc"] == B).all(), "size query: not the blocks' size"
        jobs_dec = eng.jobs_strided(src, cs, clen, dst, B, sized["tpbc"].astype(np.uint32))       # dst_cap from the size results
        f_size = lambda: eng.decompress_size(jobs_size, n)
        f_dec = lambda: eng.decompress(jobs_dec, n)
        once(f_size); once(f_dec)                                                              # warm-up
        ts, td = [], []
        for _ in range(REPS):
            ts.append(once(f_size)[0])
            ms, res = once(f_dec)
            td.append(ms)
        assert (eng.results_to_host(res)["cc"] == 0).all()
        ms_s, ms_d = statistics.median(ts), statistics.median(td)
        gib = n * B / 2 ** 30
        say("%-32s %8d | %12.1f %12.1f %8.2f | %.3f (%.3f..%.3f) / %.3f (%.3f..%.3f)" % (
            kind, n, gib / (ms_s * 1e-3), gib / (ms_d * 1e-3), ms_d / ms_s, ms_s, min(ts), max(ts), ms_d, min(td), max(td)))
        del jobs_size, jobs_dec, dst, src
        torch.cuda.empty_cache()
eng.close()
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        f.write("# tools/bench_size.py: nxz_batch_decompress_size beside nxz_batch_decompress (the engine's own route) on the same streams,\n"
                "# one process, MI355X; rates in uncompressed GiB/s, ratio = decode time / size time (above 1: the size query is the faster)\n")
        f.write("\n".join(lines) + "\n")
