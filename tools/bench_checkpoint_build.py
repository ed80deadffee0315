"""nxz_batch_checkpoint_build -- index and windows in one pass over the source -- beside what the tree needed for the same result
before it: nxz_batch_decompress_framed into a full target, then nxz_batch_checkpoint_index_fine with windows.
  shapes  64 zlib -6 streams of 16 MiB of text (the shape of profiles/r15_checkpoints_fine.txt) and 4096 streams of 1 MiB
  spans   64 KiB and 1 MiB
For every shape and span both routes write cbit / uoff / state / windows of the same size; the records and positions are compared
once.  Each route is warmed up once, then timed REPS times (device events around the asynchronous calls), the routes alternating.
Device memory is what a route holds at its peak beyond the source, which both need: its arrays -- the decode route's target
included -- and the scratch the engine grew for it, read off hipMemGetInfo around a fresh engine's first call.
No threshold is fixed: the decode route runs the workgroup kernel and may well be faster where its target fits; the build call's
claim is the memory.
Measured (MI355X, profiles/r17_checkpoint_build.txt): build / decode+index time 1.71 on 64 x 16 MiB and 2.7 on 4096 x 1 MiB;
memory 0.32 - 0.36 at a span of 64 KiB, 0.04 - 0.09 at 1 MiB.
usage: bench_checkpoint_build.py [out.txt]     -> profiles/r17_checkpoint_build.txt"""
import importlib, os, statistics, sys, zlib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
pkg = importlib.import_module("power-gzip_amd")
REPS = int(os.environ.get("REPS", "5"))
SHAPES = [tuple(int(x) for x in s.split("x")) for s in os.environ.get("SHAPES", "64x16,4096x1").split(",")]      # streams x MiB
SPANS = (65536, 1 << 20)
DISTINCT = 4
STATE = pkg.CHECKPOINT_STATE_DTYPE.itemsize
W = pkg.CHECKPOINT_WINDOW
alice = open(os.path.join(ROOT, "tests", "golden", "alice29.txt"), "rb").read()
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def plain(k, size):
    o = k * 30011 % len(alice)
    return (alice * -(-(size + o) // len(alice)))[o:o + size]


def timed(f):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def free_bytes(dev):
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info(dev)[0]


class Route:
    """a route with an engine and arrays of its own; held: device memory from before the arrays to behind the first call"""

    def __init__(self, kind, src, slot, lens, n, size, span):
        torch.cuda.empty_cache()
        self.eng = eng = pkg.Engine(0)
        dev = eng.dev
        before = free_bytes(dev)
        cap = size // (span - 257) + 2
        self.cbit = torch.zeros((n, cap + 1), dtype=torch.int64, device=dev)
        self.uoff = torch.zeros((n, cap + 1), dtype=torch.int64, device=dev)
        self.state = torch.zeros((n, (cap + 1) * STATE), dtype=torch.uint8, device=dev)
        self.windows = torch.zeros((n, cap, W), dtype=torch.uint8, device=dev)
        self.streams = torch.zeros(n * pkg.CHECKPOINT_STREAM_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        if kind == "build":
            jobs = self.jobs_without_target(src, slot, lens, n)                # dst = NULL, dst_cap = 0
            self.call = lambda: eng.checkpoint_build(pkg.FMT_ZLIB, jobs, n, span, cap, self.state, self.cbit, self.uoff, self.windows, self.streams)
        else:
            self.dst = torch.empty((n, size), dtype=torch.uint8, device=dev)
            jobs = eng.jobs_strided(src, slot, lens, self.dst, size, size)
            res = torch.empty(n * pkg.RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
            frames = torch.empty(n * pkg.FRAME_DTYPE.itemsize, dtype=torch.uint8, device=dev)

            def call():
                eng.decompress_framed(pkg.FMT_ZLIB, jobs, n, res, frames)
                return eng.checkpoint_index_fine(pkg.FMT_ZLIB, jobs, n, span, cap, self.windows, self.cbit, self.uoff, self.state, self.streams)
            self.call = call
        assert self.call()[0] == 0
        self.held = before - free_bytes(dev)
        self.st = eng.results_to_host(self.streams, pkg.CHECKPOINT_STREAM_DTYPE)[:n]
        assert (self.st["status"] == pkg.CPS_OK).all() and (self.st["out_len"] == size).all(), self.st[:4]

    def jobs_without_target(self, src, slot, lens, n):
        j = np.zeros(n, pkg.JOB_DTYPE)
        j["src"] = np.uint64(src.data_ptr()) + np.arange(n, dtype=np.uint64) * np.uint64(slot)
        j["src_len"] = lens
        j["in_adler"] = 1
        return self.eng.to_device(j)

    def close(self):
        self.eng.close()
        self.__dict__.clear()
        torch.cuda.empty_cache()


def shape_leg(n, mib):
    size = mib << 20
    texts = [plain(k, size) for k in range(DISTINCT)]
    packed = [zlib.compress(t, 6) for t in texts]
    slot = (max(map(len, packed)) + 31) & ~15
    host = np.zeros((DISTINCT, slot), np.uint8)
    for i, b in enumerate(packed):
        host[i, :len(b)] = np.frombuffer(b, np.uint8)
    src = torch.from_numpy(host).cuda().repeat(-(-n // DISTINCT), 1)[:n].contiguous()
    lens = np.tile(np.array([len(b) for b in packed], np.uint32), -(-n // DISTINCT))[:n]
    say("%d zlib -6 streams of %d MiB of text (alice29), %.1f MiB of source, median of %d" % (n, mib, n * slot / 2 ** 20, REPS))
    for span in SPANS:
        routes = {k: Route(k, src, slot, lens, n, size, span) for k in ("build", "decode+index")}
        a, b = routes["build"], routes["decode+index"]
        assert (a.st == b.st).all() and torch.equal(a.cbit, b.cbit) and torch.equal(a.uoff, b.uoff) and torch.equal(a.state, b.state)
        cnt = int(a.st["count"][0])
        assert torch.equal(a.windows, b.windows)                          # (behind the window's bytes and the stored slots: zeros in both)
        ms = {k: [] for k in routes}
        for _ in range(REPS):
            for k, r in routes.items():
                ms[k].append(timed(r.call))
        med = {k: statistics.median(v) for k, v in ms.items()}
        gib = lambda t: n * size / 2 ** 30 / (t / 1000)
        say("  span %8d, %d checkpoints a stream:" % (span, cnt))
        for k, r in routes.items():
            say("    %-13s %9.2f ms  %7.2f GiB/s of output   %9.1f MiB of device memory held" % (k, med[k], gib(med[k]), r.held / 2 ** 20))
        say("    build / decode+index: time %.2f, memory %.3f" % (med["build"] / med["decode+index"], a.held / b.held))
        for r in (a, b):
            r.close()


for n, mib in SHAPES:
    shape_leg(n, mib)
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r17_checkpoint_build.txt")
os.makedirs(os.path.dirname(out_path), exist_ok=True)
open(out_path, "w").write("\n".join(lines) + "\n")
