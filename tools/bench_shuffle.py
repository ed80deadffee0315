"""nxz_batch_shuffle / nxz_batch_unshuffle, alone and beside the codec.
(1) The pass alone: every buffer of the shape in one call, elem 2, 4, 8 (the constant paths) and 12 (the generic path), against
    nxz_copy_device of the same total bytes -- the engine's 16-bytes-a-lane copy, the roofline of a pass that reads and writes every
    byte once.  Shapes: 4096 buffers of 1 MiB and 65 536 of 64 KiB.
(2) Beside the codec: float32 random walks and bf16 N(0, 0.02) weights, 1024 buffers of 1 MiB made on the device;
    nxz_batch_deflate_streams (zlib, DHTGEN, hist_max 0) on the plain bytes against shuffle + nxz_batch_deflate_streams on the
    shuffled bytes: time and compressed bytes -- the engine's own ratio gain from the filter.
Each route is warmed up once, then all are timed in turn REPS times (a host clock around work that ends in a device synchronise) and
the medians are compared.
usage: bench_shuffle.py [out.txt] -> profiles/r26_shuffle.txt.  SHAPES=4096x1024,65536x64 picks other shapes (the first default
needs about 8.5 GiB of device memory), CODEC=1024x1024 the codec's."""
import importlib, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
pkg = importlib.import_module("power-gzip_amd")
E = pkg.engine
REPS = int(os.environ.get("REPS", "5"))
SHAPES = [tuple(int(v) for v in s.split("x")) for s in os.environ.get("SHAPES", "4096x1024,65536x64").split(",")]
CODEC = tuple(int(v) for v in os.environ.get("CODEC", "1024x1024").split("x"))
ELEMS = [2, 4, 8, 12]
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


def timed(routes):
    for f in routes.values():
        clocked(f)
    ms = {k: [] for k in routes}
    for _ in range(REPS):
        for k, f in routes.items():
            ms[k].append(clocked(f))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in ms.items()}


eng = pkg.Engine(0)


def shuffle_jobs(src, dst, n, size, elem):
    j = np.zeros(n, E.SHUFFLE_JOB_DTYPE)
    idx = np.arange(n, dtype=np.uint64) * np.uint64(size)
    j["src"], j["dst"], j["len"], j["elem"] = np.uint64(src.data_ptr()) + idx, np.uint64(dst.data_ptr()) + idx, size, elem
    return j


def pass_alone(n, kib):
    size, total = kib * 1024, n * kib * 1024
    src = torch.randint(0, 256, (total,), dtype=torch.uint8, device=eng.dev)
    dst = torch.empty(total, dtype=torch.uint8, device=eng.dev)
    status = torch.empty(n, dtype=torch.int32, device=eng.dev)

    def call(j, undo):
        def f():
            rc, _ = eng.shuffle(j, status=status, undo=undo)
            assert rc == 0, rc
        return f
    routes = {"copy": lambda: eng.copy_device(dst, src)}
    for elem in ELEMS:
        routes["sh%d" % elem] = call(shuffle_jobs(src, dst, n, size, elem), False)
        routes["un%d" % elem] = call(shuffle_jobs(dst, src, n, size, elem), True)
    m = timed(routes)
    cm = m["copy"][0]
    say("%d buffers of %d KiB; ms: median (min..max) of %d; GiB/s of source bytes; time over the copy's" % (n, kib, REPS))
    say("  %-22s %8.3f (%.3f..%.3f) %8.1f GiB/s" % ("nxz_copy_device", cm, m["copy"][1], m["copy"][2], total / cm / 1e-3 / 2 ** 30))
    for elem in ELEMS:
        for k, name in (("sh%d" % elem, "shuffle   elem %2d" % elem), ("un%d" % elem, "unshuffle elem %2d" % elem)):
            med, lo, hi = m[k]
            say("  %-22s %8.3f (%.3f..%.3f) %8.1f GiB/s  %.2f" % (name + (" (generic)" if elem == 12 else ""), med, lo, hi, total / med / 1e-3 / 2 ** 30, med / cm))
    # the pair undoes itself (the last timed route of each elem left src = unshuffle(dst); run one pair on fresh bytes)
    ref = src.clone()
    j = shuffle_jobs(src, dst, n, size, 4)
    eng.shuffle(j, status=status)
    src.zero_()
    eng.shuffle(shuffle_jobs(dst, src, n, size, 4), status=status, undo=True)
    torch.cuda.synchronize()
    assert torch.equal(src, ref) and not bool(status.any()), "unshuffle(shuffle(x)) != x"
    del src, dst, ref
    torch.cuda.empty_cache()


def beside_the_codec(n, kib):
    size, total = kib * 1024, n * kib * 1024
    gen = torch.Generator(device=eng.dev).manual_seed(26)
    data = {"float32 random walk": (torch.randn((n, size // 4), generator=gen, device=eng.dev).cumsum(1).contiguous().view(torch.uint8).reshape(-1), 4),
            "bf16 N(0, 0.02) weights": ((torch.randn((n, size // 2), generator=gen, device=eng.dev) * 0.02).to(torch.bfloat16).contiguous().view(torch.uint8).reshape(-1), 2)}
    bound = eng.deflate_stream_bound(size, 0, FMT)
    stride = (bound + 15) & ~15
    out = torch.empty(n * stride, dtype=torch.uint8, device=eng.dev)
    sh = torch.empty(total, dtype=torch.uint8, device=eng.dev)
    res = torch.empty(n * E.STREAM_RESULT_DTYPE.itemsize, dtype=torch.uint8, device=eng.dev)
    status = torch.empty(n, dtype=torch.int32, device=eng.dev)
    idx = np.arange(n, dtype=np.uint64)
    say("%d buffers of %d KiB, zlib, DHTGEN, hist_max 0; ms: median (min..max) of %d; compressed over source bytes" % (n, kib, REPS))
    for name, (src, elem) in data.items():
        def stream_jobs(buf):
            j = np.zeros(n, E.STREAM_JOB_DTYPE)
            j["src"], j["dst"] = np.uint64(buf.data_ptr()) + idx * np.uint64(size), np.uint64(out.data_ptr()) + idx * np.uint64(stride)
            j["src_len"], j["dst_cap"] = size, bound
            return j
        jp, js, jsh = stream_jobs(src), stream_jobs(sh), shuffle_jobs(src, sh, n, size, elem)

        def plain():
            rc, _ = eng.deflate_stream_jobs(FC, FMT, jp, results=res)
            assert rc == 0, rc

        def shuffled():
            rc, _ = eng.shuffle(jsh, status=status)
            assert rc == 0, rc
            rc, _ = eng.deflate_stream_jobs(FC, FMT, js, results=res)
            assert rc == 0, rc
        m = timed({"plain": plain, "shuffled": shuffled})
        sizes = {}
        for k, f in (("plain", plain), ("shuffled", shuffled)):
            clocked(f)
            r = eng.results_to_host(res, E.STREAM_RESULT_DTYPE)[:n]
            assert (r["cc"] == 0).all()
            sizes[k] = int(r["out_len"].sum())
        for k, label in (("plain", "deflate_streams"), ("shuffled", "shuffle + deflate_streams")):
            med, lo, hi = m[k]
            say("  %-24s %-26s %8.2f (%.2f..%.2f) %6.1f GiB/s  %12d bytes  %.3f" % (name, label, med, lo, hi, total / med / 1e-3 / 2 ** 30, sizes[k], sizes[k] / total))
        say("  %-24s shuffled over plain: time %.3f, compressed bytes %.3f" % (name, m["shuffled"][0] / m["plain"][0], sizes["shuffled"] / sizes["plain"]))


for n, kib in SHAPES:
    pass_alone(n, kib)
beside_the_codec(*CODEC)
eng.close()
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        f.write("\n".join(lines) + "\n")
