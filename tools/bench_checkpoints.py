"""The checkpoint calls beside what the tree could do before them.
  index   nxz_batch_checkpoint_index (positions alone, and with the windows copied out of the decoded output) beside
          nxz_batch_decompress_size_framed on the same batch of zlib streams: the same walk, a wavefront a stream.
  ranges  nxz_checkpoint_read_ranges of 1 %, 10 % and 100 % of ONE stream (one range from its middle, and the same bytes as 64
          ranges spread evenly) beside nxz_batch_decompress_framed of the whole stream, the only way to those bytes without an index.
Streams are STREAM_MIB of alice29-derived text each (zlib -6, memLevel 8: blocks of 60-100 KiB of text), checkpoints SPAN bytes
apart.  Each call is warmed up once, then timed REPS times (device events around the asynchronous calls, a host clock around the
synchronous range read), the calls alternating; rates are uncompressed GiB/s over the median.
With --fine, the fine calls (checkpoints inside blocks) beside the coarse ones instead: the two index builds on the same streams at
spans of 64 KiB and 1 MiB, each call with the arrays its own count needs; then a 4 KiB read from the middle and a whole-stream read
of ONE fixed-code stream of FIXED_MIB (64) through both indexes -- zlib's Z_FIXED stream as it is (zlib ends a block every 32 Ki
symbols), and the same tokens as ONE block (the blocks' token bits spliced behind one header: the case a coarse index cannot cut).
Measured (MI355X, profiles/r15_checkpoints_fine.txt): fine / coarse index time 0.98 and 0.97; coarse / fine read time on zlib's
stream (377 blocks, 1025 fine checkpoints) 2.70 for the 4 KiB and 2.29 for the whole stream, on the one-block stream 34.8 and 27.5.
usage: bench_checkpoints.py [out.txt]          -> profiles/r14_checkpoints.txt (the coarse calls)
       bench_checkpoints.py --fine [out.txt]   -> profiles/r15_checkpoints_fine.txt (the fine leg alone)"""
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
FINE = "--fine" in sys.argv
ARGS = [a for a in sys.argv[1:] if a != "--fine"]
eng.decompress_framed(pkg.FMT_ZLIB, jobs, NSTREAMS, res, frames)         # the outputs the windows are copied from
assert (eng.frames_to_host(frames)["status"] == pkg.FRAME_OK).all()


def coarse_leg():
    say("%d zlib -6 streams of %d MiB of text (alice29), checkpoints %d bytes apart, median of %d" % (NSTREAMS, STREAM >> 20, SPAN, REPS))
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
    out_path = ARGS[0] if ARGS else os.path.join(ROOT, "profiles", "r14_checkpoints.txt")
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    open(out_path, "w").write("\n".join(lines) + "\n")


def one_block(fz, ftext):
    """zlib's Z_FIXED stream fz with all its blocks merged into one: a block is a 3-bit header, tokens, and the 7-bit end-of-block
    code 0000000; the tokens of all blocks, bit for bit, behind one final fixed-code header (distances do not care about blocks)"""
    import checkpoint_model as M
    headers, end, _ = M.block_boundaries(fz, M.FMT_ZLIB)
    bits = np.unpackbits(np.frombuffer(fz, np.uint8), bitorder="little")
    parts = [np.array([1, 1, 0], np.uint8)]                                 # BFINAL 1, BTYPE 01
    bounds = [h for h, _ in headers] + [end[0]]
    for a, b in zip(bounds, bounds[1:]):
        assert bits[a + 1] == 1 and bits[a + 2] == 0 and not bits[b - 7:b].any()
        parts.append(bits[a + 3:b - 7])
    parts.append(np.zeros(7, np.uint8))
    body = np.packbits(np.concatenate(parts), bitorder="little").tobytes()
    one = fz[:2] + body + fz[-4:]
    assert zlib.decompress(one) == ftext
    return one, len(headers)


def fine_leg():
    STATE = pkg.CHECKPOINT_STATE_DTYPE.itemsize
    say("fine index beside the coarse index, %d zlib -6 streams of %d MiB of text (alice29), median of %d" % (NSTREAMS, STREAM >> 20, REPS))
    for span in (65536, 1 << 20):
        ccap, fcap = STREAM // span + 2, STREAM // (span - 257) + 2       # (the coarse call with the parent's own arguments)
        ccb = torch.zeros((NSTREAMS, ccap + 1), dtype=torch.int64, device=dev)
        cuo = torch.zeros((NSTREAMS, ccap + 1), dtype=torch.int64, device=dev)
        fcb = torch.zeros((NSTREAMS, fcap + 1), dtype=torch.int64, device=dev)
        fuo = torch.zeros((NSTREAMS, fcap + 1), dtype=torch.int64, device=dev)
        sta = torch.zeros((NSTREAMS, (fcap + 1) * STATE), dtype=torch.uint8, device=dev)
        legs = {"coarse": lambda: eng.checkpoint_index(pkg.FMT_ZLIB, jobs, NSTREAMS, span, ccap, None, ccb, cuo, streams),
                "fine": lambda: eng.checkpoint_index_fine(pkg.FMT_ZLIB, jobs, NSTREAMS, span, fcap, None, fcb, fuo, sta, streams)}
        counts, t = {}, {k: [] for k in legs}
        for k, f in legs.items():
            f()
            stt = eng.results_to_host(streams, pkg.CHECKPOINT_STREAM_DTYPE)
            assert (stt["status"] == pkg.CPS_OK).all(), stt[:4]
            counts[k] = int(stt["count"][0])
        for _ in range(REPS):
            for k, f in legs.items():
                t[k].append(timed(f))
        m = {k: statistics.median(v) for k, v in t.items()}
        say("  span %8d: coarse %8.2f ms (%d checkpoints a stream), fine %8.2f ms (%d)   fine / coarse = %.2f" % (span, m["coarse"], counts["coarse"], m["fine"], counts["fine"], m["fine"] / m["coarse"]))

    FIXED = int(os.environ.get("FIXED_MIB", "64")) << 20
    ftext = (alice * -(-FIXED // len(alice)))[:FIXED]
    c = zlib.compressobj(6, zlib.DEFLATED, 15, 9, zlib.Z_FIXED)
    fz = c.compress(ftext) + c.flush()
    merged, nblocks = one_block(fz, ftext)
    ftext_d = torch.from_numpy(np.frombuffer(ftext, np.uint8).copy()).to(dev)
    fout = torch.empty(FIXED, dtype=torch.uint8, device=dev)
    fdst = torch.empty(FIXED + 16, dtype=torch.uint8, device=dev)
    span = 65536
    for label, z in (("zlib's Z_FIXED stream (memLevel 9, %d blocks)" % nblocks, fz), ("the same tokens as ONE block", merged)):
        fsrc = torch.from_numpy(np.frombuffer(z + bytes(32), np.uint8).copy()).to(dev)
        fjob = eng.jobs_strided(fsrc.reshape(1, -1), fsrc.numel(), np.array([len(z)], np.uint32), fdst.reshape(1, -1), FIXED, FIXED)
        eng.decompress_framed(pkg.FMT_ZLIB, fjob, 1, res, frames)
        assert eng.frames_to_host(frames)[0]["status"] == pkg.FRAME_OK and torch.equal(fdst[:FIXED], ftext_d)
        idx = {}
        for kind in ("coarse", "fine"):
            cap = FIXED // span + 2 if kind == "coarse" else FIXED // (span - 257) + 2
            cb = torch.zeros((1, cap + 1), dtype=torch.int64, device=dev)
            uo = torch.zeros((1, cap + 1), dtype=torch.int64, device=dev)
            wi = torch.zeros((1, cap, pkg.CHECKPOINT_WINDOW), dtype=torch.uint8, device=dev)
            sta = torch.zeros((1, (cap + 1) * STATE), dtype=torch.uint8, device=dev)
            if kind == "coarse":
                eng.checkpoint_index(pkg.FMT_ZLIB, fjob, 1, span, cap, wi, cb, uo, streams)
            else:
                eng.checkpoint_index_fine(pkg.FMT_ZLIB, fjob, 1, span, cap, wi, cb, uo, sta, streams)
            s1 = eng.results_to_host(streams, pkg.CHECKPOINT_STREAM_DTYPE)[0]
            assert s1["status"] == pkg.CPS_OK and s1["out_len"] == FIXED, s1
            n1 = int(s1["count"])
            idx[kind] = (n1, cb[0, :n1 + 1].contiguous(), uo[0, :n1 + 1].contiguous(), sta[0, :(n1 + 1) * STATE].contiguous(), wi[0, :n1].contiguous())
        say("%d MiB of text, %s, span %d: %d coarse checkpoints, %d fine" % (FIXED >> 20, label, span, idx["coarse"][0], idx["fine"][0]))
        for what, rs in (("4 KiB from the middle", [(FIXED // 2, FIXED // 2 + 4096)]), ("the whole stream", [(0, FIXED)])):
            r = torch.tensor(np.array(rs, np.int64), device=dev)
            reads = {"coarse": lambda: eng.checkpoint_read_ranges(fsrc, len(z), idx["coarse"][1], idx["coarse"][2], idx["coarse"][4], r, fout),
                     "fine": lambda: eng.checkpoint_read_ranges_fine(fsrc, len(z), idx["fine"][1], idx["fine"][2], idx["fine"][3], idx["fine"][4], r, fout)}
            t, dec = {}, {}
            for k, f in reads.items():
                fout.zero_()
                rc, offs, status, out_len, decoded, _ = f()
                assert rc == 0 and bool((status == pkg.RANGE_OK).all()) and torch.equal(fout[:out_len], ftext_d[rs[0][0]:rs[0][1]])
                dec[k] = decoded
                t[k] = statistics.median(walled(f) for _ in range(REPS if z is fz else 3))
            say("  %-22s coarse %9.2f ms (%d segments), fine %9.2f ms (%d segments)   coarse / fine = %.2f" % (what, t["coarse"], dec["coarse"], t["fine"], dec["fine"], t["coarse"] / t["fine"]))
    out_path = ARGS[0] if ARGS else os.path.join(ROOT, "profiles", "r15_checkpoints_fine.txt")
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    open(out_path, "w").write("\n".join(lines) + "\n")


fine_leg() if FINE else coarse_leg()
eng.close()
