#!/usr/bin/env python3
"""Measures the shared preset dictionary of the batched interface (include/nxz_engine.h: nxz_batch_*_dict) against what a caller
had to do without it.  A measuring script only: bench.py does not run it.

Data: the corpus of tests/corpus.py, class by class: the dictionary is the first 32 KiB of the class, the records are cut
from the rest (--records of them over all classes, shared out by the classes' sizes).  Every class is a batch of its own
(one dictionary a batch); the times below are sums over the classes.  For every record size:

  ratio        compressed size with and without the dictionary (FC_COMPRESS_DHTGEN)
  compress     nxz_batch_compress_dict against nxz_batch_compress on jobs staged as [window][record] with hist_len (the
               staging itself is not timed); device bytes each way holds for its sources
  decompress   nxz_batch_decompress_dict against nxz_batch_decompress on jobs staged as [window][stream] with hist_len
  framed       nxz_batch_decompress_framed_dict on the streams packed by nxz_batch_pack_zlib_dict against decompress_dict

Every figure is the median of --runs runs of --reps calls between two events, with the lowest and highest run beside it; the two
ways of a comparison take their runs in turns.
Prints one JSON line per record size.  Usage: python tools/bench_dict.py [--records 262144] [--sizes 512,2048,8192]
"""
import argparse
import importlib
import json
import os
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

WINDOW = 32768


def timed(torch, fn, reps, runs):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / reps)
    ms.sort()
    return np.array([ms[len(ms) // 2], ms[0], ms[-1]])


def timed_pair(torch, fa, fb, reps, runs):
    """two ways to do the same thing, run by run in turns (so that a drift of clocks or of the device's state meets both)"""
    fa(); fb()
    torch.cuda.synchronize()
    ma, mb = [], []
    for _ in range(runs):
        for f, m in ((fa, ma), (fb, mb)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                f()
            e1.record()
            torch.cuda.synchronize()
            m.append(e0.elapsed_time(e1) / reps)
    ma.sort(); mb.sort()
    return np.array([ma[len(ma) // 2], ma[0], ma[-1]]), np.array([mb[len(mb) // 2], mb[0], mb[-1]])


def jobs(pkg, eng, src, src_stride, lens, dst, dst_stride, cap, hist=0):
    n = len(lens)
    j = np.zeros(n, pkg.JOB_DTYPE)
    j["src"] = np.uint64(src.data_ptr()) + np.arange(n, dtype=np.uint64) * np.uint64(src_stride)
    j["dst"] = np.uint64(dst.data_ptr()) + np.arange(n, dtype=np.uint64) * np.uint64(dst_stride)
    j["src_len"] = lens
    j["hist_len"] = hist
    j["dst_cap"] = cap
    j["in_adler"] = 1
    return eng.to_device(j)


def one_class(torch, pkg, eng, data, R, n, reps, runs):
    """one class of the corpus: its dictionary, n records of R bytes; returns the sums this class adds"""
    dict_bytes, rest = data[:WINDOW], data[WINDOW:]
    uniq = max(1, min(n, (len(rest) - R) // R))
    host = np.frombuffer(rest[:uniq * R], np.uint8).reshape(uniq, R)
    idx = torch.from_numpy(np.arange(n) % uniq).to(eng.dev)
    recs = torch.from_numpy(host.copy()).to(eng.dev)[idx].contiguous()                    # n x R, what a caller holds
    d = eng.dict_create(dict_bytes)
    W = d.deflate_window
    win = torch.from_numpy(np.frombuffer(dict_bytes[len(dict_bytes) - W:], np.uint8).copy()).to(eng.dev)
    cap = (int(eng.L.nxz_compress_bound(R)) + 512 + 15) & ~15
    lens = np.full(n, R, np.uint32)
    res = torch.empty(n * pkg.RESULT_DTYPE.itemsize, dtype=torch.uint8, device=eng.dev)
    out = {"records": n}
    # ---- compress ----
    cdst = torch.empty((n, cap), dtype=torch.uint8, device=eng.dev)
    jd = jobs(pkg, eng, recs, R, lens, cdst, cap, cap)
    fc = pkg.FC_COMPRESS_DHTGEN
    staged = torch.empty((n, W + R), dtype=torch.uint8, device=eng.dev)                   # the old way: a window per job
    staged[:, :W] = win
    staged[:, W:] = recs
    cdst2 = torch.empty((n, cap), dtype=torch.uint8, device=eng.dev)
    js = jobs(pkg, eng, staged, W + R, lens + np.uint32(W), cdst2, cap, cap, hist=W)
    res_s = torch.empty_like(res)
    out["c_dict"], out["c_staged"] = timed_pair(torch, lambda: eng.compress_dict(fc, d, jd, n, results=res),
                                                lambda: eng.compress(fc, js, n, results=res_s), reps, runs)
    rd = eng.results_to_host(res).copy()
    rs = eng.results_to_host(res_s).copy()
    ok = bool((rd["cc"] == rs["cc"]).all() and (rd["tpbc"] == rs["tpbc"]).all() and (rd["crc"] == rs["crc"]).all())
    ok = ok and bool(torch.equal(cdst[:, :int(rd["tpbc"].min())], cdst2[:, :int(rd["tpbc"].min())]))
    jn = jobs(pkg, eng, recs, R, lens, cdst2, cap, cap)
    eng.compress(fc, jn, n, results=res)
    rn = eng.results_to_host(res).copy()
    out["bytes_in"], out["bytes_dict"], out["bytes_plain"] = float(n) * R, float(rd["tpbc"].sum()), float(rn["tpbc"].sum())
    out["src_mem_dict"], out["src_mem_staged"] = float(n) * R + WINDOW, float(n) * (W + R)
    del cdst2, staged, js, jn
    # ---- decompress: the streams of compress_dict ----
    eng.compress_dict(fc, d, jd, n, results=res)
    clen = rd["tpbc"].astype(np.uint32)
    back = torch.empty((n, R), dtype=torch.uint8, device=eng.dev)
    ju = jobs(pkg, eng, cdst, cap, clen, back, R, R)
    res2 = torch.empty_like(res)
    eng.decompress_dict(d, ju, n, results=res2)
    reasons = eng.wg_reasons()
    ok = ok and bool((eng.results_to_host(res2)["cc"] == 0).all()) and bool(torch.equal(back, recs)) and reasons is not None and reasons["handed_back"] == 0
    staged = torch.empty((n, WINDOW + cap), dtype=torch.uint8, device=eng.dev)             # [inflate window][stream]
    staged[:, :WINDOW] = torch.from_numpy(np.frombuffer(dict_bytes, np.uint8).copy()).to(eng.dev)
    staged[:, WINDOW:] = cdst
    back2 = torch.zeros_like(back)
    res3 = torch.empty_like(res)
    jv = jobs(pkg, eng, staged, WINDOW + cap, clen + np.uint32(WINDOW), back2, R, R, hist=WINDOW)
    out["d_dict"], out["d_staged"] = timed_pair(torch, lambda: eng.decompress_dict(d, ju, n, results=res2),
                                                lambda: eng.decompress(jv, n, results=res3), reps, runs)
    ok = ok and bool((eng.results_to_host(res3)["cc"] == 0).all()) and bool(torch.equal(back2, recs))
    del staged, jv, back2
    # ---- framed ----
    packed = torch.empty(n * 10 + n * max(cap, R + 5) + 64, dtype=torch.uint8, device=eng.dev)
    offs = eng.pack_zlib_dict(6, d, jd, res, n, packed)
    torch.cuda.synchronize()
    o = offs.cpu().numpy()
    jf = np.zeros(n, pkg.JOB_DTYPE)
    jf["src"] = np.uint64(packed.data_ptr()) + o[:n].astype(np.uint64)
    jf["src_len"] = np.diff(o).astype(np.uint32)
    jf["dst"] = np.uint64(back.data_ptr()) + np.arange(n, dtype=np.uint64) * np.uint64(R)
    jf["dst_cap"], jf["in_adler"] = R, 1
    jf = eng.to_device(jf)
    frames = torch.empty(n * pkg.FRAME_DTYPE.itemsize, dtype=torch.uint8, device=eng.dev)
    back.zero_()
    out["d_framed"] = timed(torch, lambda: eng.decompress_framed_dict(pkg.FMT_ZLIB, d, jf, n, results=res2, frames=frames), reps, runs)
    ok = ok and bool((eng.frames_to_host(frames)["status"] == pkg.FRAME_OK).all()) and bool(torch.equal(back, recs))
    m = packed[:int(o[1])].cpu().numpy().tobytes()
    ok = ok and zlib.decompressobj(zdict=dict_bytes).decompress(m) == host[0].tobytes()
    out["correct"] = ok
    d.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=1 << 18)
    ap.add_argument("--sizes", default="512,2048,8192")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--runs", type=int, default=5)
    args = ap.parse_args()
    import torch
    import corpus
    pkg = importlib.import_module("power-gzip_amd")
    for k in ("NXZ_INFLATE_LANES_MIN", "NXZ_INFLATE_CUT", "NXZ_INFLATE_WG", "NXZ_INFLATE_WG_MAX", "NXZ_FUSED_GEN", "NXZ_DICT_WG_MIN"):
        os.environ.pop(k, None)
    eng = pkg.Engine(0)
    name, blocks, _ = corpus.load(65536)
    classes = {}
    for cls, _, b in blocks:
        classes.setdefault(cls, []).append(b)
    classes = {c: b"".join(v) for c, v in classes.items() if sum(map(len, v)) >= WINDOW + 65536}
    total = sum(len(v) for v in classes.values())
    for R in (int(x) for x in args.sizes.split(",")):
        acc = None
        for c, data in sorted(classes.items()):
            n = max(256, args.records * len(data) // total)
            r = one_class(torch, pkg, eng, data, R, n, args.reps, args.runs)
            torch.cuda.empty_cache()
            if acc is None:
                acc = r
            else:
                for k, v in r.items():
                    acc[k] = (acc[k] and v) if k == "correct" else acc[k] + v
        t = lambda k: {"median_ms": round(float(acc[k][0]), 3), "low_ms": round(float(acc[k][1]), 3), "high_ms": round(float(acc[k][2]), 3)}
        gib = lambda k: round(acc["bytes_in"] / (acc[k][0] * 1e-3) / 2 ** 30, 2)
        print(json.dumps({
            "record_bytes": R, "records": acc["records"], "classes": len(classes), "corpus": name, "correct": acc["correct"],
            "ratio_without_dict": round(acc["bytes_in"] / acc["bytes_plain"], 3), "ratio_with_dict": round(acc["bytes_in"] / acc["bytes_dict"], 3),
            "compress_dict": t("c_dict"), "compress_staged": t("c_staged"), "compress_dict_gibs": gib("c_dict"), "compress_staged_gibs": gib("c_staged"),
            "compress_dict_over_staged": round(float(acc["c_staged"][0] / acc["c_dict"][0]), 4),
            "source_bytes_dict": int(acc["src_mem_dict"]), "source_bytes_staged": int(acc["src_mem_staged"]),
            "decompress_dict": t("d_dict"), "decompress_staged": t("d_staged"), "decompress_dict_gibs": gib("d_dict"), "decompress_staged_gibs": gib("d_staged"),
            "decompress_dict_over_staged": round(float(acc["d_staged"][0] / acc["d_dict"][0]), 4),
            "framed_dict": t("d_framed"), "framed_over_raw_dict": round(float(acc["d_dict"][0] / acc["d_framed"][0]), 4)}), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
