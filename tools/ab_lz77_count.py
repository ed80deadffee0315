"""What the symbol counts cost inside the LZ77 kernel: the headline's buffers and job count (bench.run_corpus), timed by
the engine's own HIP events (bench.timed_compress), legs alternating, RUNS runs of STEPS steps each:

  A  FC_COMPRESS_DHTGEN                        the LZ77 stage with counts
  B  FC_COMPRESS_DHT, one table for all jobs   lz77_kernel<false, false, false>: the same parse, no counts

  python tools/ab_lz77_count.py [--corpus-jobs J] [--steps K] [--warmup W] [--runs R] [--inkernel]

The difference A - B of the LZ77 stage is what counting costs on the route A takes.  --inkernel adds leg
  C  FC_COMPRESS_DHTGEN with NXZ_LZ77_COUNT_INKERNEL=1   lz77_kernel<true, false, false>, the counts inside the kernel
(in a build that counts in nxzsc::count_kernel by default, A against C is that kernel against the fused counting).
Under `rocprofv3 --kernel-trace --stats -- python tools/ab_lz77_count.py --runs 1 --steps 3` the per-kernel averages."""
import argparse
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def universal_table(O, block):
    """a table with a code for every symbol, from one block's counts"""
    tok, nt = O.lz77(block, 0)
    ll, d = O.counts(tok, nt)
    for i in range(286):
        ll[i] = max(ll[i], 1)
    for i in range(30):
        d[i] = max(d[i], 1)
    return O.dhtgen(ll, d)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--corpus-jobs", type=int, default=262144)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--inkernel", action="store_true")
    args = ap.parse_args()

    import numpy as np
    import torch

    import bench
    import corpus
    import oracle_lib as O
    pkg = importlib.import_module("power-gzip_amd")
    eng = pkg.Engine(0)

    # the headline's buffers (bench.run_corpus)
    name, blocks, _ = corpus.load(bench.BLOCK)
    uniq = len(blocks)
    rep = max(1, -(-args.corpus_jobs // uniq))
    n = uniq * rep
    host = np.zeros((uniq, bench.BLOCK), np.uint8)
    lens_u = np.array([len(b) for _, _, b in blocks], np.uint32)
    for i, (_, _, b) in enumerate(blocks):
        host[i, :len(b)] = np.frombuffer(b, np.uint8)
    src = torch.from_numpy(host).to(eng.dev).repeat(rep, 1)
    dst = torch.empty((n, bench.STRIDE_OUT), dtype=torch.uint8, device=eng.dev)
    jobs = eng.jobs_strided(src, bench.BLOCK, np.tile(lens_u, rep), dst, bench.STRIDE_OUT, bench.STRIDE_OUT, dht_index=0)
    res = torch.empty(n * pkg.RESULT_DTYPE.itemsize, dtype=torch.uint8, device=eng.dev)
    bits, dhtlen = universal_table(O, blocks[0][2])
    arr = np.zeros(1, pkg.DHT_DTYPE)
    arr["dhtlen"][0] = dhtlen
    arr["dht"][0, :len(bits)] = np.frombuffer(bits, np.uint8)
    dht = eng.to_device(arr)

    class WithTable:
        """eng.compress with the caller's table, behind the signature bench.timed_compress calls"""
        L, ctx, dev = eng.L, eng.ctx, eng.dev

        @staticmethod
        def compress(fc, jobs, n, results=None):
            return eng.compress(fc, jobs, n, results=results, dht=dht, ntables=1)

    legs = [("A dhtgen", pkg.FC_COMPRESS_DHTGEN, eng, None), ("B dht", pkg.FC_COMPRESS_DHT, WithTable, None)]
    if args.inkernel:
        legs.append(("C dhtgen, counts in the LZ77 kernel", pkg.FC_COMPRESS_DHTGEN, eng, "1"))
    print("corpus %s, %d jobs (%d unique blocks), %d runs of %d steps, warm-up %d" % (name, n, uniq, args.runs, args.steps, args.warmup), flush=True)
    rows = {leg[0]: [] for leg in legs}
    for run in range(args.runs):
        for what, fc, e, knob in legs:
            saved = os.environ.pop("NXZ_LZ77_COUNT_INKERNEL", None)
            if knob is not None:
                os.environ["NXZ_LZ77_COUNT_INKERNEL"] = knob
            try:
                ms, st, launches = bench.timed_compress(torch, e, fc, jobs, n, res, args.steps, args.warmup if run == 0 else 1)
            finally:
                os.environ.pop("NXZ_LZ77_COUNT_INKERNEL", None)
                if saved is not None:
                    os.environ["NXZ_LZ77_COUNT_INKERNEL"] = saved
            r = eng.results_to_host(res)
            bad = int(((r["cc"] != 0) & (r["cc"] != 64)).sum())
            row = {"leg": what, "run": run + 1, "ms_per_step": round(ms, 3), "lz77_ms": round(st[0], 3), "dhtgen_ms": round(st[1], 3),
                   "entropy_ms": round(st[2], 3), "launches": launches, "jobs_with_errors": bad}
            rows[what].append(row)
            print(json.dumps(row), flush=True)
    med = {}
    for what, rs in rows.items():
        lz = sorted(x["lz77_ms"] for x in rs)
        med[what] = lz[len(lz) // 2]
        print("%-40s lz77 ms a step: median %.3f, spread %.3f (max - min)" % (what, med[what], lz[-1] - lz[0]))
    print("A - B of the LZ77 stage: %.3f ms a step" % (med["A dhtgen"] - med["B dht"]))
    if args.inkernel:
        print("C - A of the LZ77 stage: %.3f ms a step" % (med["C dhtgen, counts in the LZ77 kernel"] - med["A dhtgen"]))
    eng.close()


if __name__ == "__main__":
    main()
