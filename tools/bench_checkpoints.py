"""The checkpoint calls beside what the tree could do before them.
  index   nxz_batch_checkpoint_index (positions alone, and with the windows copied out of the decoded output) beside
          nxz_batch_decompress_size_framed on the same batch of zlib streams: the same walk, a wavefront a stream.
  ranges  nxz_checkpoint_read_ranges of 1 %, 10 % and 100 % of ONE stream (one range from its middle, and the same bytes as 64
          ranges spread evenly) beside nxz_batch_decompress_framed of the whole stream, the only way to those bytes without an index.
Streams are STREAM_MIB of alice29-derived text each (zlib -6, memLevel 8: blocks of 60-100 KiB of text), checkpoints SPAN bytes
apart.  Each call is warmed up once, then timed REPS times (device events around the asynchronous calls, a host clock around the
synchronous range read), the calls alternating; rates are uncompressed GiB/s over the median.
usage: bench_checkpoints.py [out.txt]  -> profiles/r14_checkpoints.txt"""
import importlib, os, statistics, sys, time, zlib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
pkg = importlib.import_module("power-gzip_amd")
REPS = int(os.environ.get("REPS", "7"))
STREAM = int(os.environ.get("STREAM_MIB", "16")) << 20
NSTREAMS = int(os.environ.get("STREAMS", "64"))
SPAN = int(os.environ.get("SPAN", "65536"))
DISTINCT = 4
alice = open(os.path.join(ROOT, "tests", "golden", "alice29.txt"), "rb").read()
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def plain(k):
    """STREAM bytes of the text from a start that moves with k"""
    o = k * 30011 % len(alice)
    reps = -(-(STREAM + o) // len(alice))
    return (alice * reps)[o:o + STREAM]


def timed(f):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def walled(f):
    torch.cuda.synchronize()
    t = time.perf_counter()
    f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1000


eng = pkg.Engine(0)
dev = eng.dev
texts = [plain(k) for k in range(DISTINCT)]
packed = [zlib.compress(t, 6) for t in texts]
slot = (max(map(len, packed)) + 31) & ~15
host = np.zeros((DISTINCT, slot), np.uint8)
for i, b in enumerate(packed):
    host[i, :len(b)] = np.frombuffer(b, np.uint8)
src = torch.from_numpy(host).to(dev).repeat(-(-NSTREAMS // DISTINCT), 1)[:NSTREAMS].contiguous()
lens = np.tile(np.array([len(b) for b in packed], np.uint32), -(-NSTREAMS // DISTINCT))[:NSTREAMS]
dst = torch.empty((NSTREAMS, STREAM), dtype=torch.uint8, device=dev)
jobs = eng.jobs_strided(src, slot, lens, dst, STREAM, STREAM)
res = torch.empty(NSTREAMS * pkg.RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
frames = torch.empty(NSTREAMS * pkg.FRAME_DTYPE.itemsize, dtype=torch.uint8, device=dev)
cp_cap = STREAM // SPAN + 2
cbit = torch.zeros((NSTREAMS, cp_cap + 1), dtype=torch.int64, device=dev)
uoff = torch.zeros((NSTREAMS, cp_cap + 1), dtype=torch.int64, device=dev)
windows = torch.zeros((NSTREAMS, cp_cap, pkg.CHECKPOINT_WINDOW), dtype=torch.uint8, device=dev)
streams = torch.zeros(NSTREAMS * pkg.CHECKPOINT_STREAM_DTYPE.itemsize, dtype=torch.uint8, device=dev)

say("%d zlib -6 streams of %d MiB of text (alice29), checkpoints %d bytes apart, median of %d" % (NSTREAMS, STREAM >> 20, SPAN, REPS))
eng.decompress_framed(pkg.FMT_ZLIB, jobs, NSTREAMS, res, frames)         # the outputs the windows are copied from
assert (eng.frames_to_host(frames)["status"] == pkg.FRAME_OK).all()
calls = {
    "size": lambda: eng.decompress_size_framed(pkg.FMT_ZLIB, jobs, NSTREAMS, None, res, frames),
    "index": lambda: eng.checkpoint_index(pkg.FMT_ZLIB, jobs, NSTREAMS, SPAN, cp_cap, None, cbit, uoff, streams),
    "index+windows": lambda: eng.checkpoint_index(pkg.FMT_ZLIB, jobs, NSTREAMS, SPAN, cp_cap, windows, cbit, uoff, streams),
}
for f in calls.values():
    f()
st = eng.results_to_host(streams, pkg.CHECKPOINT_STREAM_DTYPE)
assert (st["status"] == pkg.CPS_OK).all() and (st["out_len"] == STREAM).all(), st[:4]
ms = {k: [] for k in calls}
for _ in range(REPS):
    for k, f in calls.items():
        ms[k].append(timed(f))
med = {k: statistics.median(v) for k, v in ms.items()}
gib = lambda nbytes, t: nbytes / 2 ** 30 / (t / 1000)
say("index build, %d checkpoints a stream:" % int(st["count"][0]))
for k in calls:
    say("  %-14s %8.2f ms  %7.1f GiB/s of output walked   (%.2f of the size call's time)" % (k, med[k], gib(NSTREAMS * STREAM, med[k]), med[k] / med["size"]))

# ---- ranges of stream 0 -------------------------------------------------------------------------------------------------------
cnt = int(st["count"][0])
c0, u0, w0 = cbit[0, :cnt + 1].contiguous(), uoff[0, :cnt + 1].contiguous(), windows[0, :cnt].contiguous()
s0, l0 = src[0], int(lens[0])
one = eng.jobs_strided(src, slot, lens[:1], dst, STREAM, STREAM)
out = torch.empty(STREAM, dtype=torch.uint8, device=dev)
text = torch.from_numpy(np.frombuffer(texts[0], np.uint8).copy()).to(dev)
whole = lambda: eng.decompress_framed(pkg.FMT_ZLIB, one, 1, res, frames)
whole()
t_whole = statistics.median(timed(whole) for _ in range(REPS))
say("ranges of one stream (%d segments); the whole stream by nxz_batch_decompress_framed: %.2f ms, %.2f GiB/s" % (cnt, t_whole, gib(STREAM, t_whole)))
say("  %5s %7s | %9s %8s %9s %9s | %s" % ("share", "ranges", "bytes", "segments", "ms", "GiB/s", "whole-stream decode's time over the read's"))
for pct in (1, 10, 100):
    nbytes = STREAM * pct // 100
    for nr in (1, 64):
        if nr == 1:
            b = (STREAM - nbytes) // 2
            rs = [(b, b + nbytes)]
        else:
            step, each = STREAM // nr, nbytes // nr
            rs = [(k * step, k * step + each) for k in range(nr)]
        r = torch.tensor(np.array(rs, np.int64), device=dev)
        read = lambda: eng.checkpoint_read_ranges(s0, l0, c0, u0, w0, r, out)
        rc, offs, status, out_len, decoded, _ = read()
        assert rc == 0 and out_len == sum(e - b for b, e in rs) and bool((status == pkg.RANGE_OK).all())
        o = offs.cpu().numpy()
        for k, (b, e) in enumerate(rs):
            assert torch.equal(out[o[k]:o[k + 1]], text[b:e])
        t = statistics.median(walled(read) for _ in range(REPS))
        say("  %4d%% %7d | %9d %8d %9.2f %9.2f | %.2f" % (pct, nr, out_len, decoded, t, gib(out_len, t), t_whole / t))
say("(a range read stages [window][source bytes] of every touched segment and decodes the segments a stream per wavefront, side by side;")
say(" the whole-stream decode is one stream on the stream-per-workgroup route)")
eng.close()
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r14_checkpoints.txt")
os.makedirs(os.path.dirname(out_path), exist_ok=True)
open(out_path, "w").write("\n".join(lines) + "\n")
