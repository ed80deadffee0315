"""nxz_batch_inflate_streams_part beside the routes that exist without it, on zlib -6 streams of the corpus' bytes:
(f)  nxz_batch_decompress_framed: every stream whole, one call;
(p1) the part call with every stream as ONE FIRST part: no window and no tail, so nothing is staged -- what differs from (f) is the
     open and close kernels and the empty staging launch;
(q4, q16) every stream handed over in 4 / 16 parts (equal shares of its compressed bytes), a call a part, ALL calls queued and ONE
     wait at the end; the outputs lie end to end (prev + prev_len == dst), every part behind the first is staged.  Where each part's
     target begins is known up front from a pass that is not timed -- a caller that does not know it gives every part a target of
     its own;
(r4, r16) the only route there is today for the same parts: nxz_batch_decompress with resume jobs.  After every part the host waits,
     reads results[] (sfbt, subc, tebc, spbc, the checksums), works out the undecoded tail, and builds the next part's jobs and
     layout: [window][tail][next part] contiguous in a slot of device memory, two device-to-device copies a stream issued from the
     host (the table of an open dynamic block stays in the call's dht_io slot from job to job).
For (q) the tool also says how many bytes the route stages (the window and the part of every part behind the first) and what it
costs over (f), so that the cost can be held against the bytes moved.
The corpus bytes, tiled, as N streams of KIB KiB of output; the distinct streams are compressed on the host (zlib level 6) and
replicated on the device.  Each route is warmed up once, then all are timed in turn REPS times (a host clock around work that ends
in a device synchronise) and the medians are compared.  All routes' outputs are held against the plain bytes once, outside the clock.
usage: bench_inflate_part.py [out.txt] -> profiles/r25_inflate_part.txt.  SHAPE=streams x KiB picks another shape (the default
needs about 18 GiB of device memory); REPS, SPLITS likewise."""
import ctypes as C
import importlib, os, statistics, sys, time, zlib
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
FMT = E.FMT_ZLIB
WINDOW, TAIL = 32768, 288
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
t = torch
_, blocks, _ = corpus.load(B)
plain = b"".join(b for _, _, b in blocks if len(b) == B)
size = KIB * 1024
U = max(1, min(N, len(plain) // size))                               # distinct streams
units = [plain[u * size:(u + 1) * size] if len(plain) >= size else (plain * (size // len(plain) + 1))[:size] for u in range(U)]
comps = [zlib.compress(d, 6) for d in units]
cstride = (max(len(c) for c in comps) + 16 + 15) & ~15
clen = np.array([len(comps[i % U]) for i in range(N)], np.int64)
# the compressed streams on the device: stream i at i * cstride + 1 (an odd address: sources have any alignment)
h = np.zeros((U, cstride), np.uint8)
for u, c in enumerate(comps):
    h[u, 1:1 + len(c)] = np.frombuffer(c, np.uint8)
d_units = t.from_numpy(h).to(eng.dev)
src = d_units.repeat(-(-N // U), 1)[:N].contiguous().view(-1)
want = t.from_numpy(np.frombuffer(b"".join(units), np.uint8).copy()).to(eng.dev).view(U, size)
ostride = size + 64
idx = np.arange(N, dtype=np.uint64)
src0 = np.uint64(src.data_ptr()) + idx * np.uint64(cstride) + np.uint64(1)


def new_out():
    return t.empty(N * ostride, dtype=t.uint8, device=eng.dev)


def check_out(out, what):
    got = out.view(N, ostride)[:, :size]
    for u in range(U):
        assert bool((got[u::U] == want[u][None, :]).all()), "%s: other bytes than the plain ones" % what


# ---- (f) the framed call ----
out_f = new_out()
jf = np.zeros(N, E.JOB_DTYPE)
jf["src"], jf["dst"] = src0, np.uint64(out_f.data_ptr()) + idx * np.uint64(ostride)
jf["src_len"], jf["dst_cap"], jf["in_adler"] = clen, ostride, 1
d_jf = eng.to_device(jf)
res_f = t.empty(N * E.RESULT_DTYPE.itemsize, dtype=t.uint8, device=eng.dev)
frames_f = t.empty(N * E.FRAME_DTYPE.itemsize, dtype=t.uint8, device=eng.dev)


def f():
    eng.decompress_framed(FMT, d_jf, N, results=res_f, frames=frames_f)


# ---- (p1, q) the part call ----
out_p = new_out()
carry = t.zeros(N * E.INFLATE_CARRY_DTYPE.itemsize, dtype=t.uint8, device=eng.dev)
res_p = t.empty(N * E.INFLATE_PART_RESULT_DTYPE.itemsize, dtype=t.uint8, device=eng.dev)


def part_bounds(parts):
    """[parts + 1, N]: where each part begins in its stream's compressed bytes"""
    return np.stack([clen * k // parts for k in range(parts + 1)])


def part_job(at, k, done_k):
    """part k of every stream: its share of the compressed bytes, its target behind the done_k output bytes in front of it"""
    j = np.zeros(N, E.INFLATE_PART_JOB_DTYPE)
    j["src"] = src0 + at[k].astype(np.uint64)
    j["src_len"] = at[k + 1] - at[k]
    j["dst"] = np.uint64(out_p.data_ptr()) + idx * np.uint64(ostride) + done_k.astype(np.uint64)
    j["dst_cap"] = ostride - done_k
    keep = np.minimum(done_k, WINDOW)
    j["prev"] = np.where(keep > 0, j["dst"] - keep.astype(np.uint64), np.uint64(0))
    j["prev_len"] = keep
    j["flags"] = E.PART_FIRST if k == 0 else 0
    return j


def parts_route(jobs):
    def g():
        for j in jobs:
            rc, _ = eng.inflate_stream_parts(FMT, j, carry, results=res_p)
            assert rc == 0, rc
    return g


def plan(parts):
    """the pass that is not timed: the parts one after the other with a wait behind each, to learn where each part's output begins.
    -> the parts' jobs"""
    done, at, jobs = np.zeros(N, np.int64), part_bounds(parts), []
    for k in range(parts):
        jobs.append(part_job(at, k, done))
        rc, _ = eng.inflate_stream_parts(FMT, jobs[-1], carry, results=res_p)
        assert rc == 0, rc
        r = eng.results_to_host(res_p, E.INFLATE_PART_RESULT_DTYPE)[:N]
        want_status = E.INFLATE_PART_DONE if k == parts - 1 else E.INFLATE_PART_MORE
        assert (r["status"] == want_status).all(), "part %d of %d: statuses %s" % (k, parts, sorted(set(r["status"].tolist())))
        done = done + r["out_len"].astype(np.int64)
    assert (done == size).all()
    return jobs


# ---- (r) today's route: resume jobs built by the host between the parts ----
# A stream's slot: its history ends at byte WINDOW of the slot and the source goes behind it.  The job begins at the 16-byte boundary
# at or below the history's first byte; the bytes between count as history (hist_len) and are never reached.  The jobs carry
# NXZ_JOB_SUSPEND_WHEN_FULL as the host loop of nxz_stream.cpp's do.
out_r = new_out()
slot = (WINDOW + TAIL + cstride + 64 + 15) & ~15
slots = t.zeros(N * slot, dtype=t.uint8, device=eng.dev)
res_r = t.empty(N * E.RESULT_DTYPE.itemsize, dtype=t.uint8, device=eng.dev)
dht_r = t.zeros(N * E.DHT_DTYPE.itemsize, dtype=t.uint8, device=eng.dev)
# the copies a C caller issues: hipMemcpyDtoDAsync of the HIP runtime this process has loaded (any alignment, any length)
_hip_path = next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line)
_hip = C.CDLL(_hip_path)
_hip.hipMemcpyDtoDAsync.restype = C.c_int
_hip.hipMemcpyDtoDAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
eng.L.nxz_batch_decompress.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]


def host_route(parts):
    at = part_bounds(parts)
    at[0] = 2                                                          # (the zlib header: the host's to skip)
    out0, slot0, s0 = out_r.data_ptr(), slots.data_ptr(), src.data_ptr()
    copy, ctx, stream = _hip.hipMemcpyDtoDAsync, eng.ctx, eng.stream_handle()

    def g():
        pos = at[0].copy()                                             # the byte of its source every stream stands at (tail included)
        total = np.zeros(N, np.int64)
        resume = np.zeros(N, np.uint32)
        crc, adler = np.zeros(N, np.uint32), np.ones(N, np.uint32)
        for k in range(parts):
            w = np.minimum(total, WINDOW)
            pad = (WINDOW - w) & 15
            n_src = at[k + 1] - pos
            j = np.zeros(N, E.JOB_DTYPE)
            if k == 0:
                pad = np.zeros(N, np.int64)
                j["src"] = src0 + pos.astype(np.uint64)
            else:
                base = slot0 + np.arange(N, dtype=np.int64) * slot + (WINDOW - w)
                for i in range(N):
                    if w[i]:
                        rc = copy(int(base[i]), out0 + i * ostride + int(total[i] - w[i]), int(w[i]), stream)
                        assert rc == 0, rc
                    rc = copy(int(base[i] + w[i]), s0 + i * cstride + 1 + int(pos[i]), int(n_src[i]), stream)
                    assert rc == 0, rc
                j["src"] = (base - pad).astype(np.uint64)
            j["dst"] = np.uint64(out0) + idx * np.uint64(ostride) + total.astype(np.uint64)
            j["src_len"], j["hist_len"], j["dst_cap"] = pad + w + n_src, pad + w, ostride - total
            j["in_crc"], j["in_adler"], j["resume"], j["reserved"] = crc, adler, resume, pkg.JOB_SUSPEND_WHEN_FULL
            d_j = eng.to_device(j)
            rc = eng.L.nxz_batch_decompress(ctx, d_j.data_ptr(), N, res_r.data_ptr(), dht_r.data_ptr(), stream)
            assert rc == 0, rc
            r = eng.results_to_host(res_r)[:N]                         # the host wait
            if not np.isin(r["cc"], (0, 3)).all():
                i = int(np.flatnonzero(~np.isin(r["cc"], (0, 3)))[0])
                raise RuntimeError("(r%d) part %d: completion codes %s; stream %d: job %s result %s" %
                                   (parts, k, sorted(set(r["cc"].tolist())), i, j[i], r[i]))
            assert (r["spbc"] == j["src_len"]).all(), "(r%d) part %d: a part was not taken whole" % (parts, k)
            back = (r["subc"].astype(np.int64) + 7) // 8
            pos = at[k + 1] - back
            total = total + r["tpbc"]
            crc, adler = r["crc"].copy(), r["adler"].copy()
            stored = (r["sfbt"] & 0xe) == 0x8
            resume = (np.where(stored, r["tebc"], 0) | (r["sfbt"] & 15) << 16 | (r["subc"] & 7) << 20).astype(np.uint32)
        assert (total == size).all() and ((r["sfbt"] & 0x100) != 0).all()
    return g


routes = {"f": f, "p1": parts_route(plan(1))}
staged = {}
for parts in SPLITS:
    jobs = plan(parts)
    routes["q%d" % parts] = parts_route(jobs)
    routes["r%d" % parts] = host_route(parts)
    staged[parts] = int(sum(int(j["prev_len"].astype(np.int64).sum()) + int(j["src_len"].astype(np.int64).sum()) for j in jobs[1:]))
for g in routes.values():                                              # (a route that breaks ends the run: no comparison goes missing quietly)
    clocked(g)
check_out(out_f, "(f)")
check_out(out_p, "(q%d)" % SPLITS[-1])
check_out(out_r, "(r%d)" % SPLITS[-1])
clocked(routes["p1"])
check_out(out_p, "(p1)")
rf, ff = eng.results_to_host(res_f)[:N], eng.results_to_host(frames_f, E.FRAME_DTYPE)[:N]
rp = eng.results_to_host(res_p, E.INFLATE_PART_RESULT_DTYPE)[:N]
assert (rp["status"] == E.INFLATE_PART_DONE).all() and (rp["in_used"] == ff["end"]).all() and (rp["out_len"] == rf["tpbc"]).all()
assert (rp["crc"] == rf["crc"]).all() and (rp["adler"] == rf["adler"]).all(), "the part call and the framed call disagree about a whole stream"
ms = {k: [] for k in routes}
for _ in range(REPS):
    for k, g in routes.items():
        ms[k].append(clocked(g))
total_out, total_in = N * size, int(clen.sum())
say("%d streams of %d KiB of output (%d distinct), zlib -6, %.1f MiB compressed; ms per route: median (min..max) of %d, GiB/s of output, and the ratio"
    % (N, KIB, U, total_in / 2 ** 20, REPS))
names = {"f": "nxz_batch_decompress_framed", "p1": "one FIRST part"}
for parts in SPLITS:
    names["q%d" % parts] = "%d parts, queued, one wait" % parts
    names["r%d" % parts] = "%d parts, resume jobs by the host" % parts
fm = statistics.median(ms["f"])
for k, name in names.items():
    med, lo, hi = statistics.median(ms[k]), min(ms[k]), max(ms[k])
    ref = "(f)" if k[0] != "r" else "(q%s)" % k[1:]
    refm = fm if k[0] != "r" else statistics.median(ms["q" + k[1:]])
    say("(%s) %-36s %9.2f (%.2f..%.2f)  %6.1f GiB/s  %.3f of %s" % (k, name, med, lo, hi, total_out / med / 1e-3 / 2 ** 30, med / refm, ref))
for parts in SPLITS:
    over = statistics.median(ms["q%d" % parts]) - fm
    say("(q%d) stages %.1f MiB (windows and parts behind the first) and costs %.2f ms more than (f): %.1f GiB/s if all of it were the copy"
        % (parts, staged[parts] / 2 ** 20, over, staged[parts] / max(over, 1e-6) / 1e-3 / 2 ** 30))
eng.close()
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as fh:
        fh.write("\n".join(lines) + "\n")
