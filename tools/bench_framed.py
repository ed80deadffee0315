#!/usr/bin/env python3
"""Measures the device-side zlib / gzip framing (include/nxz_engine.h) against the raw batch it wraps.  A measuring script only:
bench.py does not run it.

  framed   nxz_batch_decompress_framed on the zlib -6 streams of the corpus chunks (the chunks bench.py's inflate_zlib6 leg
           uses), kept with their zlib framing, against nxz_batch_decompress on the same streams' deflate bytes, at 65 536
           and 262 548 streams
  unpack   nxz_batch_unpack_gzip on a BGZF image of >= 1 GiB made of the corpus on the device (compress batch +
           nxz_batch_pack_gzip), against nxz_batch_decompress of the same members' payloads in place
  discover the discovery alone (nxz_batch_unpack_gzip with max_members = 0 returns -E2BIG once it has counted the members),
           events around it

Prints one JSON line per measurement.  Usage: python tools/bench_framed.py [--reps 5] [--image-gib 1.05] [--sizes 65536,262548]
"""
import argparse
import errno
import importlib
import json
import os
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

BLOCK = 65536
MEMBER = 65280          # BGZF members of this much source keep every output offset 16-byte aligned


def timed(torch, fn, reps):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def jobs_for(pkg, eng, src_ptrs, src_lens, dst, dst_stride, cap):
    n = len(src_ptrs)
    j = np.zeros(n, pkg.JOB_DTYPE)
    j["src"] = src_ptrs
    j["src_len"] = src_lens
    j["dst"] = np.uint64(dst.data_ptr()) + np.arange(n, dtype=np.uint64) * np.uint64(dst_stride)
    j["dst_cap"] = cap
    j["in_adler"] = 1
    return eng.to_device(j)


def framed_leg(torch, pkg, eng, raw, n, reps):
    streams = [zlib.compress(b, 6) for b in raw]
    uniq = len(streams)
    stride = (max(len(s) for s in streams) + 64 + 15) & ~15
    host = np.zeros((uniq, stride), np.uint8)
    body = np.zeros((uniq, stride), np.uint8)
    for i, s in enumerate(streams):
        host[i, :len(s)] = np.frombuffer(s, np.uint8)
        body[i, :len(s) - 6] = np.frombuffer(s[2:-4], np.uint8)
    src, bsrc = torch.from_numpy(host).to(eng.dev), torch.from_numpy(body).to(eng.dev)
    idx = np.arange(n) % uniq
    dst = torch.empty((n, BLOCK), dtype=torch.uint8, device=eng.dev)
    clen = np.array([len(s) for s in streams], np.uint32)[idx]
    fj = jobs_for(pkg, eng, np.uint64(src.data_ptr()) + idx.astype(np.uint64) * np.uint64(stride), clen, dst, BLOCK, BLOCK)
    rj = jobs_for(pkg, eng, np.uint64(bsrc.data_ptr()) + idx.astype(np.uint64) * np.uint64(stride), clen - 6, dst, BLOCK, BLOCK)
    res = torch.empty(n * pkg.RESULT_DTYPE.itemsize, dtype=torch.uint8, device=eng.dev)
    frames = torch.empty(n * pkg.FRAME_DTYPE.itemsize, dtype=torch.uint8, device=eng.dev)
    ulen = np.array([len(b) for b in raw], np.float64)[idx].sum()
    ms_raw = timed(torch, lambda: eng.decompress(rj, n, results=res), reps)
    ms_fr = timed(torch, lambda: eng.decompress_framed(pkg.FMT_ZLIB, fj, n, results=res, frames=frames), reps)
    f = eng.frames_to_host(frames)
    r = eng.results_to_host(res)
    ok = bool((f["status"] == pkg.FRAME_OK).all() and (r["cc"] == 0).all())
    ok = ok and all(dst[i, :len(raw[idx[i]])].cpu().numpy().tobytes() == raw[idx[i]] for i in range(0, n, max(1, n // 64)))
    gib = lambda ms: round(ulen / (ms * 1e-3) / 2 ** 30, 2)
    return {"leg": "framed_zlib6", "streams": n, "raw_ms": round(ms_raw, 3), "framed_ms": round(ms_fr, 3), "raw_gibs": gib(ms_raw),
            "framed_gibs": gib(ms_fr), "ratio": round(ms_raw / ms_fr, 4), "target": 0.97, "correct": ok}


def unpack_legs(torch, pkg, eng, raw, gib_target, reps):
    # corpus chunks of MEMBER bytes, compressed on the device (own exact tables) and packed as BGZF members
    data = b"".join(raw)
    chunks = [data[i:i + MEMBER] for i in range(0, len(data) - MEMBER + 1, MEMBER)]
    uniq = len(chunks)
    host = np.frombuffer(b"".join(chunks), np.uint8).reshape(uniq, MEMBER)
    src = torch.from_numpy(host.copy()).to(eng.dev)
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
        return packed, offs.cpu().numpy(), idx
    probe, po, _ = pack(min(uniq, 512))
    per = po[-1] / (len(po) - 1)
    del probe
    m = int(gib_target * 2 ** 30 / per) + 1
    packed, offs, idx = pack(m)
    size = int(offs[m])
    dst = torch.empty(m * MEMBER, dtype=torch.uint8, device=eng.dev)
    out = {}
    # the whole call
    rcs = []
    ms_un = timed(torch, lambda: rcs.append(eng.unpack_gzip(packed, size, dst, m)[0]), reps)
    rc, d = eng.unpack_gzip(packed, size, dst, m)
    f = eng.frames_to_host(d["frames"])
    ok = rc == 0 and all(r == 0 for r in rcs) and d["members"] == m and d["out_len"] == m * MEMBER and bool((f["status"] == pkg.FRAME_OK).all())
    ok = ok and all(dst[k * MEMBER:(k + 1) * MEMBER].cpu().numpy().tobytes() == chunks[idx[k]] for k in range(0, m, max(1, m // 32)))
    # the raw batch of the same members: their payloads in place (sources at any alignment), outputs MEMBER apart
    pay = np.uint64(packed.data_ptr()) + offs[:m].astype(np.uint64) + np.uint64(18)
    rj = jobs_for(pkg, eng, pay, (np.diff(offs) - 26).astype(np.uint32), dst, MEMBER, MEMBER)
    res = torch.empty(m * pkg.RESULT_DTYPE.itemsize, dtype=torch.uint8, device=eng.dev)
    ms_raw = timed(torch, lambda: eng.decompress(rj, m, results=res), reps)
    gib = lambda ms: round(m * MEMBER / (ms * 1e-3) / 2 ** 30, 2)
    out["unpack"] = {"leg": "unpack_gzip", "image_bytes": size, "members": m, "raw_ms": round(ms_raw, 3), "unpack_ms": round(ms_un, 3),
                     "raw_gibs": gib(ms_raw), "unpack_gibs": gib(ms_un), "ratio": round(ms_raw / ms_un, 4), "target": 0.9, "correct": ok}
    # discovery alone
    drc = []
    ms_d = timed(torch, lambda: drc.append(eng.unpack_gzip(packed, size, dst, 0)[0]), reps)
    out["discover"] = {"leg": "discover", "image_bytes": size, "members": m, "ms": round(ms_d, 3), "target_ms": 1.0,
                       "correct": all(r == -errno.E2BIG for r in drc)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="65536,262548")
    ap.add_argument("--image-gib", type=float, default=1.05)
    ap.add_argument("--skip", default="", help="comma list of legs to skip: framed, unpack")
    args = ap.parse_args()
    import torch
    import corpus
    pkg = importlib.import_module("power-gzip_amd")
    for k in ("NXZ_INFLATE_LANES_MIN", "NXZ_INFLATE_CUT", "NXZ_INFLATE_WG", "NXZ_INFLATE_WG_MAX"):
        os.environ.pop(k, None)
    eng = pkg.Engine(0)
    name, blocks, _ = corpus.load(BLOCK)
    raw = [b for _, _, b in blocks]
    skip = set(args.skip.split(","))
    if "framed" not in skip:
        for n in (int(x) for x in args.sizes.split(",")):
            r = framed_leg(torch, pkg, eng, raw, n, args.reps)
            r["corpus"] = name
            print(json.dumps(r), flush=True)
            torch.cuda.empty_cache()
    if "unpack" not in skip:
        for v in unpack_legs(torch, pkg, eng, raw, args.image_gib, args.reps).values():
            v["corpus"] = name
            print(json.dumps(v), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
