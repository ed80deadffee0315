"""nxz_batch_decompress_verify_framed -- checksums and trailer checks with no decode target -- beside the routes around it, on the
zlib -6 streams of tools/bench_checkpoints.py / bench_checkpoint_build.py:
  verify      nxz_batch_decompress_verify_framed, dst = NULL
  decode      nxz_batch_decompress_framed into full targets: the one way to the same verdict before
  size        nxz_batch_decompress_size_framed: the walk alone
  walk+ring   nxz_batch_checkpoint_build with one span larger than any stream: the walk plus the ring, no checksum passes
  shapes      64 streams of 16 MiB of text and 4096 streams of 1 MiB
The verify's records and frames are compared with the decode's once.  Each route has an engine of its own, is warmed up once, then
timed REPS times (device events around the asynchronous calls), the routes alternating.  Device memory is what a route holds at its
peak beyond the source, which all need: its arrays -- the decode's targets included -- and the scratch the engine grew for it, read
off hipMemGetInfo around a fresh engine's first call.
No threshold is fixed: the decode runs the workgroup kernel and is expected to be the faster one where its targets fit; the verify
call's claim is the memory.  The file says how much slower it is, and what share of its time the checksum passes add over walk+ring.
usage: bench_verify.py [out.txt]     -> profiles/r18_verify.txt"""
import importlib, os, statistics, sys, zlib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
pkg = importlib.import_module("power-gzip_amd")
REPS = int(os.environ.get("REPS", "5"))
SHAPES = [tuple(int(x) for x in s.split("x")) for s in os.environ.get("SHAPES", "64x16,4096x1").split(",")]      # streams x MiB
DISTINCT = 4
KINDS = ("verify", "decode", "size", "walk+ring")
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

    def __init__(self, kind, src, slot, lens, n, size):
        torch.cuda.empty_cache()
        self.eng = eng = pkg.Engine(0)
        dev = eng.dev
        before = free_bytes(dev)
        self.res = torch.zeros(n * pkg.RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        self.frames = torch.zeros(n * pkg.FRAME_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        j = np.zeros(n, pkg.JOB_DTYPE)                                        # dst = NULL
        j["src"] = np.uint64(src.data_ptr()) + np.arange(n, dtype=np.uint64) * np.uint64(slot)
        j["src_len"], j["in_adler"], j["dst_cap"] = lens, 1, 0xffffffff
        jobs = eng.to_device(j)
        if kind == "verify":
            self.call = lambda: eng.decompress_verify_framed(pkg.FMT_ZLIB, jobs, n, None, self.res, self.frames)
        elif kind == "size":
            self.call = lambda: eng.decompress_size_framed(pkg.FMT_ZLIB, jobs, n, None, self.res, self.frames)
        elif kind == "decode":
            self.dst = torch.empty((n, size), dtype=torch.uint8, device=dev)
            djobs = eng.jobs_strided(src, slot, lens, self.dst, size, size)
            self.call = lambda: eng.decompress_framed(pkg.FMT_ZLIB, djobs, n, self.res, self.frames)
        else:
            span, cap = 2 * size, 1
            self.cbit = torch.zeros((n, cap + 1), dtype=torch.int64, device=dev)
            self.uoff = torch.zeros((n, cap + 1), dtype=torch.int64, device=dev)
            self.state = torch.zeros((n, (cap + 1) * pkg.CHECKPOINT_STATE_DTYPE.itemsize), dtype=torch.uint8, device=dev)
            self.windows = torch.zeros((n, cap, pkg.CHECKPOINT_WINDOW), dtype=torch.uint8, device=dev)
            self.streams = torch.zeros(n * pkg.CHECKPOINT_STREAM_DTYPE.itemsize, dtype=torch.uint8, device=dev)
            j["dst_cap"] = 0
            bjobs = eng.to_device(j)
            self.call = lambda: eng.checkpoint_build(pkg.FMT_ZLIB, bjobs, n, span, cap, self.state, self.cbit, self.uoff, self.windows, self.streams)
        self.call()
        self.held = before - free_bytes(dev)
        if kind == "walk+ring":
            st = eng.results_to_host(self.streams, pkg.CHECKPOINT_STREAM_DTYPE)[:n]
            assert (st["status"] == pkg.CPS_OK).all() and (st["out_len"] == size).all(), st[:4]
        else:
            self.r, self.f = eng.results_to_host(self.res).copy(), eng.frames_to_host(self.frames).copy()
            assert (self.f["status"] == pkg.FRAME_OK).all() and (self.r["cc"] == 0).all() and (self.r["tpbc"] == size).all(), (kind, self.r[:4])

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
    routes = {k: Route(k, src, slot, lens, n, size) for k in KINDS}
    v, d = routes["verify"], routes["decode"]
    assert (v.r == d.r).all() and (v.f == d.f).all()                         # records and frames, checksums included
    for i in range(DISTINCT):
        assert int(v.r["adler"][i]) == zlib.adler32(texts[i]) and int(v.r["crc"][i]) == zlib.crc32(texts[i])
    ms = {k: [] for k in routes}
    for _ in range(REPS):
        for k, r in routes.items():
            ms[k].append(timed(r.call))
    med = {k: statistics.median(t) for k, t in ms.items()}
    gib = lambda t: n * size / 2 ** 30 / (t / 1000)
    for k, r in routes.items():
        say("    %-10s %9.2f ms (%.2f - %.2f)  %7.2f GiB/s of output   %9.1f MiB of device memory held" % (k, med[k], min(ms[k]), max(ms[k]), gib(med[k]), r.held / 2 ** 20))
    say("    verify / decode: time %.2f, memory %.3f;  verify / size: time %.2f;  the checksum passes: %.0f %% of the verify's time (over walk+ring)"
        % (med["verify"] / med["decode"], v.held / d.held, med["verify"] / med["size"], 100 * (med["verify"] - med["walk+ring"]) / med["verify"]))
    for r in list(routes.values()):
        r.close()


for n, mib in SHAPES:
    shape_leg(n, mib)
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r18_verify.txt")
os.makedirs(os.path.dirname(out_path), exist_ok=True)
open(out_path, "w").write("\n".join(lines) + "\n")
