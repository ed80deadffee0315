#!/usr/bin/env python3
"""Measures BGZF random access (include/nxz_engine.h: nxz_bgzf_index, nxz_bgzf_read_ranges) on the BGZF image tools/bench_framed.py
unpacks (>= 1 GiB of corpus chunks of 65 280 bytes, compressed and packed as members on the device).  A measuring script only:
bench.py does not run it.

  index     nxz_bgzf_index alone, against the discovery of nxz_batch_unpack_gzip (max_members = 0: -E2BIG once counted)
  whole     the whole image as one range, and as one range per member, against nxz_batch_unpack_gzip
  uoff      1 / 64 / 4 096 random ranges of 4 KiB, 64 KiB and 1 MiB, index given
  voff      the same ranges in virtual offsets

Times are per call (the call is synchronous), GiB/s count the bytes delivered.  Prints one JSON line per measurement.
Usage: python tools/bench_bgzf_ranges.py [--reps 5] [--image-gib 1.05]
"""
import argparse
import errno
import importlib
import json
import os
import random
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_framed import BLOCK, MEMBER, jobs_for, timed   # noqa: E402


def host_timed(torch, fn, reps):
    """wall time of a synchronous call (its own waits included)"""
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps


def make_image(torch, pkg, eng, raw, gib_target):
    data = b"".join(raw)
    chunks = [data[i:i + MEMBER] for i in range(0, len(data) - MEMBER + 1, MEMBER)]
    uniq = len(chunks)
    src = torch.from_numpy(np.frombuffer(b"".join(chunks), np.uint8).reshape(uniq, MEMBER).copy()).to(eng.dev)
    cap = 73856

    def pack(m):
        idx = np.arange(m) % uniq
        cdst = torch.empty((m, cap), dtype=torch.uint8, device=eng.dev)
        j = jobs_for(pkg, eng, np.uint64(src.data_ptr()) + idx.astype(np.uint64) * np.uint64(MEMBER), np.full(m, MEMBER, np.uint32), cdst, cap, cap)
        res, _ = eng.compress(pkg.FC_COMPRESS_DHTGEN, j, m)
        packed = torch.empty(m * (MEMBER + 40) + 64, dtype=torch.uint8, device=eng.dev)
        offs = eng.pack_gzip(j, res, m, packed)
        torch.cuda.synchronize()
        del cdst, res, j
        return packed, offs.cpu().numpy()
    probe, po = pack(min(uniq, 512))
    per = po[-1] / (len(po) - 1)
    del probe
    m = int(gib_target * 2 ** 30 / per) + 1
    packed, offs = pack(m)
    del src
    torch.cuda.empty_cache()
    return packed, int(offs[m]), m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--image-gib", type=float, default=1.05)
    args = ap.parse_args()
    import torch
    import corpus
    pkg = importlib.import_module("power-gzip_amd")
    for k in ("NXZ_INFLATE_LANES_MIN", "NXZ_INFLATE_CUT", "NXZ_INFLATE_WG", "NXZ_INFLATE_WG_MAX", "NXZ_BGZF_CHUNK"):
        os.environ.pop(k, None)
    eng = pkg.Engine(0)
    name, blocks, _ = corpus.load(BLOCK)
    packed, size, m = make_image(torch, pkg, eng, [b for _, _, b in blocks], args.image_gib)
    U = m * MEMBER
    gib = lambda nbytes, ms: round(nbytes / (ms * 1e-3) / 2 ** 30, 2)
    emit = lambda d: print(json.dumps(dict(d, corpus=name, image_bytes=size, members=m)), flush=True)

    # (a) the index, against the discovery
    drc = []
    ms_d = timed(torch, lambda: drc.append(eng.unpack_gzip(packed, size, packed, 0)[0]), args.reps)
    ms_i = host_timed(torch, lambda: eng.bgzf_index(packed, size, m + 1), args.reps)
    coff, uoff = eng.bgzf_index(packed, size, m + 1)
    ok = len(coff) == m + 1 and int(uoff[-1]) == U and int(coff[-1]) == size and all(r == -errno.E2BIG for r in drc)
    emit({"leg": "index", "ms": round(ms_i, 3), "discover_ms": round(ms_d, 3), "correct": ok})

    # (b) the whole image: unpack, one range, one range per member
    dst_u = torch.empty(U + 16, dtype=torch.uint8, device=eng.dev)
    ms_un = host_timed(torch, lambda: eng.unpack_gzip(packed, size, dst_u, m), args.reps)
    dst_r = torch.empty(U + 16, dtype=torch.uint8, device=eng.dev)
    ones = torch.tensor([[0, U]], dtype=torch.int64, device=eng.dev)
    cuts = uoff.clone()
    per_member = torch.stack([cuts[:-1], cuts[1:]], 1).contiguous()
    for label, rng in (("whole_one_range", ones), ("whole_range_per_member", per_member)):
        rcs = []
        ms = host_timed(torch, lambda: rcs.append(eng.bgzf_read_ranges(packed, size, coff, uoff, rng, pkg.RANGE_UOFF, dst_r)[0]), args.reps)
        st = eng.bgzf_read_ranges(packed, size, coff, uoff, rng, pkg.RANGE_UOFF, dst_r)[2]
        ok = all(r == 0 for r in rcs) and bool((st == 0).all()) and bool(torch.equal(dst_r[:U], dst_u[:U]))
        emit({"leg": label, "ranges": rng.shape[0], "ms": round(ms, 3), "gibs": gib(U, ms), "unpack_ms": round(ms_un, 3),
              "unpack_gibs": gib(U, ms_un), "ratio": round(ms_un / ms, 4), "target": 0.85, "correct": ok})

    # (c) / (d) random ranges, index given
    rnd = random.Random(1)
    co, uo = coff.cpu().numpy().astype(np.uint64), uoff.cpu().numpy().astype(np.uint64)
    for n in (1, 64, 4096):
        for rsize in (4096, 65536, 1 << 20):
            b = np.array([rnd.randrange(0, U - rsize) for _ in range(n)], np.uint64)
            e = b + np.uint64(rsize)
            touched = len(set().union(*(range(int(x) // MEMBER, (int(y) - 1) // MEMBER + 1) for x, y in zip(b, e))))
            # virtual offsets: the member that holds b (every member holds MEMBER bytes here) and the one that ends at e or holds it
            jb, je = b // np.uint64(MEMBER), (e - np.uint64(1)) // np.uint64(MEMBER)
            vb = co[jb.astype(np.int64)] << np.uint64(16) | (b - uo[jb.astype(np.int64)])
            ve = co[je.astype(np.int64)] << np.uint64(16) | (e - uo[je.astype(np.int64)])
            dst = torch.empty(n * rsize + 16, dtype=torch.uint8, device=eng.dev)
            for kind, (x, y) in ((pkg.RANGE_UOFF, (b, e)), (pkg.RANGE_VOFF, (vb, ve))):
                rng = torch.tensor(np.stack([x, y], 1).view(np.int64), device=eng.dev)
                rcs = []
                ms = host_timed(torch, lambda: rcs.append(eng.bgzf_read_ranges(packed, size, coff, uoff, rng, kind, dst)[0]), args.reps)
                rc, offs, st, out_len, decoded, _ = eng.bgzf_read_ranges(packed, size, coff, uoff, rng, kind, dst)
                ok = rc == 0 and all(r == 0 for r in rcs) and out_len == n * rsize and decoded == touched and bool((st == 0).all())
                for i in range(0, n, max(1, n // 16)):
                    ok = ok and bool(torch.equal(dst[i * rsize:(i + 1) * rsize], dst_u[int(b[i]):int(e[i])]))
                emit({"leg": "uoff" if kind == pkg.RANGE_UOFF else "voff", "ranges": n, "range_bytes": rsize, "members_decoded": decoded,
                      "ms": round(ms, 3), "gibs": gib(n * rsize, ms), "vs_unpack": round(ms / ms_un, 4), "correct": ok})
            del dst
    eng.close()


if __name__ == "__main__":
    main()
