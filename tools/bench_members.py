"""Multi-member gzip jobs beside what the framed call could do with the same members: nxz_batch_gzip_members_size (the index walk) and
nxz_batch_gzip_members_decode on jobs of 1 / 16 / 1024 members of alice29-derived data, against nxz_batch_decompress_framed on the
same members as separate jobs, each source and target 16-byte aligned.  Every job holds about TOTAL_MIB / jobs of plain text, so the
three shapes decode the same bytes.  Each call is warmed up once, then timed REPS times with device events, the calls alternating; the
rate is uncompressed GiB/s over the median.  usage: bench_members.py [out.txt]  -> profiles/r12_members.txt"""
import importlib, os, statistics, struct, sys, zlib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
pkg = importlib.import_module("power-gzip_amd")
REPS = int(os.environ.get("REPS", "7"))
TOTAL = int(os.environ.get("TOTAL_MIB", "256")) << 20
MEMBER = int(os.environ.get("MEMBER_BYTES", "16384"))          # plain bytes a member
SHAPES = [int(x) for x in os.environ.get("MEMBERS", "1,16,1024").split(",")]
alice = open(os.path.join(ROOT, "tests", "golden", "alice29.txt"), "rb").read()
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def member(k):
    """member k: MEMBER bytes of the text from a start that moves with k (64 distinct members, reused)"""
    o = (k % 64) * 2000
    d = (alice + alice)[o:o + MEMBER]
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    return b"\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\xff" + c.compress(d) + c.flush() + struct.pack("<II", zlib.crc32(d), len(d))


def timed(f):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def place(bufs, slot):
    host = np.zeros((len(bufs), slot), np.uint8)
    for i, b in enumerate(bufs):
        host[i, :len(b)] = np.frombuffer(b, np.uint8)
    return host


eng = pkg.Engine(0)
dev = eng.dev
pool = [member(k) for k in range(64)]
say("members of %d plain bytes (alice29, zlib -6), %d MiB of output a batch, median of %d" % (MEMBER, TOTAL >> 20, REPS))
say("%8s %8s | %10s %10s %10s | %8s %8s | %s" % ("members", "jobs", "index", "decode", "framed", "idx+dec", "/framed", "ms: index / decode / framed"))
for per in SHAPES:
    njobs = max(1, TOTAL // (per * MEMBER))
    distinct = min(njobs, 32)
    job_bufs = [b"".join(pool[(j * 7 + k) % 64] for k in range(per)) for j in range(distinct)]
    slot = (max(len(b) for b in job_bufs) + 31) & ~15
    src = torch.from_numpy(place(job_bufs, slot)).to(dev).repeat(-(-njobs // distinct), 1)[:njobs].contiguous()
    out_job = per * MEMBER
    dst = torch.empty((njobs, out_job), dtype=torch.uint8, device=dev)
    lens = np.tile(np.array([len(b) for b in job_bufs], np.uint32), -(-njobs // distinct))[:njobs]
    jobs = eng.jobs_strided(src, slot, lens, dst, out_job, out_job)
    # the same members as separate framed jobs, sources and targets 16-byte aligned
    nm = njobs * per
    mslot = (max(len(m) for m in pool) + 31) & ~15
    order = np.array([(j % distinct * 7 + k) % 64 for j in range(njobs) for k in range(per)])
    msrc = torch.from_numpy(place(pool, mslot)).to(dev)[torch.from_numpy(order).to(dev)].contiguous()
    mdst = torch.empty((nm, MEMBER), dtype=torch.uint8, device=dev)
    mjobs = eng.jobs_strided(msrc, mslot, np.array([len(pool[o]) for o in order], np.uint32), mdst, MEMBER, MEMBER)
    members = torch.empty(njobs * per * pkg.GZIP_MEMBER_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    streams = torch.empty(njobs * pkg.GZIP_STREAM_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    res = torch.empty(nm * pkg.RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    frames = torch.empty(nm * pkg.FRAME_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    calls = {
        "index": lambda: eng.gzip_members_size(jobs, njobs, per, members, streams),
        "decode": lambda: eng.gzip_members_decode(jobs, njobs, per, members, streams),
        "framed": lambda: eng.decompress_framed(pkg.FMT_GZIP, mjobs, nm, res, frames),
    }
    for f in calls.values():
        f()
    torch.cuda.synchronize()
    s = eng.results_to_host(streams, pkg.GZIP_STREAM_DTYPE)
    fr = eng.frames_to_host(frames)
    assert (s["status"] == pkg.GZS_OK).all() and (s["out_len"] == out_job).all() and (fr["status"] == pkg.FRAME_OK).all()
    assert bool((dst.view(-1)[:nm * MEMBER].view(nm, MEMBER) == mdst).all())
    ms = {k: [] for k in calls}
    for _ in range(REPS):
        for k, f in calls.items():                          # (the decode reads what the index of the same turn wrote)
            ms[k].append(timed(f))
    med = {k: statistics.median(v) for k, v in ms.items()}
    gib = lambda t: njobs * out_job / 2 ** 30 / (t / 1000)
    say("%8d %8d | %10.1f %10.1f %10.1f | %8.1f %8.2f | %.2f / %.2f / %.2f" % (
        per, njobs, gib(med["index"]), gib(med["decode"]), gib(med["framed"]), gib(med["index"] + med["decode"]),
        med["framed"] / (med["index"] + med["decode"]), med["index"], med["decode"], med["framed"]))
say("(GiB/s of output; idx+dec: both passes; /framed: the framed call's time over theirs -- above 1 the two passes are faster)")
eng.close()
out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r12_members.txt")
os.makedirs(os.path.dirname(out), exist_ok=True)
open(out, "w").write("\n".join(lines) + "\n")
