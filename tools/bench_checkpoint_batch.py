"""nxz_batch_checkpoint_read_ranges -- ranges over all the streams of an indexed batch in ONE call -- beside what the tree had for the
same bytes before it: a loop of nxz_checkpoint_read_ranges_fine calls, one a stream, each with its own two host waits.
  shapes  64 zlib -6 streams of 16 MiB of text with one 4 KiB range each (64 ranges); 4096 streams of 1 MiB with one 4 KiB range
          each; 4096 streams of 1 MiB with the whole stream as the range
  spans   64 KiB and 1 MiB (nxz_batch_checkpoint_build with states)
Both routes read through the same index into targets of the same size; the bytes are compared equal first (and, for the 4 KiB
ranges, with the plain text).  Each route is warmed up once (its scratch is grown), then timed REPS times, the routes alternating:
device events around the route on the engine's stream, and the wall clock beside them -- both routes are synchronous, the loop's
time is mostly its host waits.  No threshold is fixed: the yardstick is the loop in the same run.
Measured (MI355X, profiles/r22_checkpoint_batch.txt): batched / loop 0.017 on 64 x 16 MiB with 4 KiB ranges, 0.001 - 0.004 on
4096 x 1 MiB with 4 KiB ranges, 0.004 - 0.006 on 4096 x 1 MiB with whole streams; the batched call is slower nowhere.
usage: bench_checkpoint_batch.py [out.txt]     -> profiles/r22_checkpoint_batch.txt"""
import ctypes as C, importlib, os, random, statistics, sys, time, zlib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
pkg = importlib.import_module("power-gzip_amd")
REPS = int(os.environ.get("REPS", "5"))
SHAPES = [(int(s.split("x")[0]), int(s.split("x")[1]), s.split("x")[2]) for s in os.environ.get("SHAPES", "64x16x4k,4096x1x4k,4096x1xall").split(",")]
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
    t0 = time.perf_counter()
    e0.record()
    f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), (time.perf_counter() - t0) * 1000


def shape_leg(eng, n, mib, what):
    size = mib << 20
    dev = eng.dev
    texts = [plain(k, size) for k in range(DISTINCT)]
    packed = [zlib.compress(t, 6) for t in texts]
    slot = (max(map(len, packed)) + 31) & ~15
    host = np.zeros((DISTINCT, slot), np.uint8)
    for i, b in enumerate(packed):
        host[i, :len(b)] = np.frombuffer(b, np.uint8)
    src = torch.from_numpy(host).to(dev).repeat(-(-n // DISTINCT), 1)[:n].contiguous()
    lens = np.tile(np.array([len(b) for b in packed], np.uint32), -(-n // DISTINCT))[:n]
    j = np.zeros(n, pkg.JOB_DTYPE)
    j["src"] = np.uint64(src.data_ptr()) + np.arange(n, dtype=np.uint64) * np.uint64(slot)
    j["src_len"] = lens
    j["in_adler"] = 1
    jobs = eng.to_device(j)
    rnd = random.Random(n + mib)
    each = size if what == "all" else 4096
    begin = [0 if what == "all" else rnd.randrange(size - each) for _ in range(n)]
    say("%d zlib -6 streams of %d MiB of text (alice29), one range of %d bytes a stream, median of %d" % (n, mib, each, REPS))
    for span in SPANS:
        cap = size // (span - 257) + 2
        rc, cbit, uoff, state, windows, streams = eng.checkpoint_build(pkg.FMT_ZLIB, jobs, n, span, cap)
        st = eng.results_to_host(streams, pkg.CHECKPOINT_STREAM_DTYPE)[:n]
        assert rc == 0 and (st["status"] == pkg.CPS_OK).all() and (st["out_len"] == size).all(), st[:4]
        q = np.zeros(n, pkg.BATCH_RANGE_DTYPE)
        q["job"] = np.arange(n)
        q["begin"] = begin
        q["end"] = np.array(begin) + each
        ranges = eng.to_device(q)
        pairs = torch.tensor(np.stack([q["begin"], q["end"]], 1).astype(np.int64), device=dev)
        dst_b = torch.zeros(n * each, dtype=torch.uint8, device=dev)
        dst_l = torch.zeros(n * each, dtype=torch.uint8, device=dev)
        offs_l = torch.zeros((n, 2), dtype=torch.int64, device=dev)
        stat_l = torch.zeros(n, dtype=torch.int32, device=dev)
        out_len, decoded = C.c_uint64(), C.c_uint64()
        got = {}

        def batched():
            rc, offs, status, total, dec, _ = eng.checkpoint_read_ranges_batch(jobs, n, cap, cbit, uoff, state, windows, streams, ranges, dst=dst_b)
            assert rc == 0 and total == n * each, (rc, total)
            got["batched"] = (status, dec)

        def loop():
            h, L, dec = eng.stream_handle(), eng.L, 0
            for i in range(n):
                nidx = int(st["count"][i]) + 1
                rc = L.nxz_checkpoint_read_ranges_fine(eng.ctx, int(j["src"][i]), int(lens[i]), cbit.data_ptr() + i * (cap + 1) * 8, uoff.data_ptr() + i * (cap + 1) * 8,
                                                       state.data_ptr() + i * (cap + 1) * STATE, windows.data_ptr() + i * cap * W, nidx,
                                                       pairs.data_ptr() + i * 16, 1, dst_l.data_ptr() + i * each, each, offs_l.data_ptr() + i * 16,
                                                       stat_l.data_ptr() + i * 4, C.byref(out_len), C.byref(decoded), h)
                assert rc == 0 and out_len.value == each, (i, rc, out_len.value)
                dec += decoded.value
            got["loop"] = (stat_l, dec)
        routes = {"batched": batched, "loop": loop}
        for f in routes.values():                                            # warm-up: the scratch of both routes is grown here
            f()
        torch.cuda.synchronize()
        assert torch.equal(dst_b, dst_l) and int(got["batched"][0].abs().sum()) == 0 and int(got["loop"][0].abs().sum()) == 0
        assert got["batched"][1] == got["loop"][1]
        back = dst_b.view(n, each)[:DISTINCT, :4096].cpu().numpy()
        for i in range(DISTINCT):
            assert back[i].tobytes() == texts[i][begin[i]:begin[i] + 4096], i
        ms = {k: [] for k in routes}
        for _ in range(REPS):
            for k, f in routes.items():
                ms[k].append(timed(f))
        ev = {k: statistics.median(x[0] for x in v) for k, v in ms.items()}
        wall = {k: statistics.median(x[1] for x in v) for k, v in ms.items()}
        say("  span %8d, %d checkpoints a stream, %d segments inflated:" % (span, int(st["count"][0]), got["batched"][1]))
        for k in routes:
            say("    %-8s %10.2f ms by events  %10.2f ms wall   %8.2f GiB/s of output" % (k, ev[k], wall[k], n * each / 2 ** 30 / (wall[k] / 1000)))
        say("    batched / loop: events %.3f, wall %.3f%s" % (ev["batched"] / ev["loop"], wall["batched"] / wall["loop"],
                                                             "   (the batched call is SLOWER here)" if wall["batched"] > wall["loop"] else ""))
        del cbit, uoff, state, windows, dst_b, dst_l
        torch.cuda.empty_cache()


engine = pkg.Engine(0)
for n_, mib_, what_ in SHAPES:
    shape_leg(engine, n_, mib_, what_)
engine.close()
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r22_checkpoint_batch.txt")
os.makedirs(os.path.dirname(out_path), exist_ok=True)
open(out_path, "w").write("\n".join(lines) + "\n")
