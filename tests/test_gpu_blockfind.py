"""GPU tests (-m gpu) of the block search of the one-stream inflate, called directly: nxz_launch_find_blocks from
power-gzip_amd/libnxz_blockfind_probe.so -- the object file the engine ships, linked without the engine's version script --
over the hand-built headers of tests/blockfind_cases.py, compared with tests/blockfind_model.py: the first header of every
segment exactly, the three further ones exactly where the second kernel does the segment (tests/blockfind_model.py
segment_class; tests/test_blockfind_model_host.py asserts that every segment of every case is one the model speaks for).

The launcher reads its settings once a process: the default (segments of 1 KiB for these streams, two kernels) runs here,
segments of 512, 2048 and 8192 bytes and the one-kernel form each in a child process of its own, one after the other.
The stream lies at every offset from a 16-byte boundary the cases name, with poison and no zeros behind it; `first` and the
scratch area are poisoned and have canaries around them.

And one stream of hand-built blocks through nxz_inflate_stream, the tenth inflate route, which the hand-built family
(tests/test_gpu_deflate_handmade.py) does not reach."""
import ctypes as C
import importlib
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":                       # a child process: no conftest has set the path
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))

import blockfind_cases as Cs
import blockfind_model as M
import deflate_handmade as H

pytestmark = pytest.mark.gpu
PROBE = os.path.join(ROOT, "power-gzip_amd", "libnxz_blockfind_probe.so")
GUARD = 16


def probe():
    import torch  # noqa: F401  (first: the library then shares torch's HIP runtime, as the engine does -- power-gzip_amd/engine.py)
    torch.cuda.init()
    L = C.CDLL(PROBE)
    L.nxz_blockfind_segment.restype = C.c_uint32
    L.nxz_blockfind_segment.argtypes = [C.c_uint64]
    L.nxz_blockfind_scratch.restype = C.c_size_t
    L.nxz_blockfind_scratch.argtypes = [C.c_uint32]
    L.nxz_launch_find_blocks.restype = C.c_int
    L.nxz_launch_find_blocks.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    return L


def search(L, c, S, two=True):
    """-> what is wrong with the search's answer for case c, a line each"""
    import torch
    n = len(c.src)
    assert L.nxz_blockfind_segment(n) == S
    nseg = (n + S - 1) // S
    buf = torch.full((n + 64,), Cs.POISON, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    buf[c.offset:c.offset + n] = torch.from_numpy(np.frombuffer(c.src, np.uint8).copy()).cuda()
    nfirst = nseg * (1 + M.MORE)
    first = torch.full((nfirst + 2 * GUARD,), 0x5a5a5a5a5a5a5a5a, dtype=torch.int64, device="cuda")
    nscr = L.nxz_blockfind_scratch(nseg)
    assert nscr == nseg * (M.LEFT_MAX + 2) * 2
    scr = torch.full((nscr + 2 * GUARD,), 0x5a, dtype=torch.uint8, device="cuda")
    rc = L.nxz_launch_find_blocks(buf.data_ptr() + c.offset, n, c.first_bit, first.data_ptr() + 8 * GUARD, nseg, scr.data_ptr() + GUARD, None)
    torch.cuda.synchronize()
    assert rc == 0, (c.name, rc)
    f, s = first.cpu().numpy().view(np.uint64), scr.cpu().numpy()
    bad = Cs.check(c, S, f[GUARD:GUARD + nfirst], two=two)
    if not ((f[:GUARD] == 0x5a5a5a5a5a5a5a5a).all() and (f[GUARD + nfirst:] == 0x5a5a5a5a5a5a5a5a).all()):
        bad.append("%s: written outside `first`" % c.name)
    if not ((s[:GUARD] == 0x5a).all() and (s[GUARD + nscr:] == 0x5a).all()):
        bad.append("%s: written outside the scratch area" % c.name)
    if not (buf[:c.offset].cpu().numpy() == Cs.POISON).all() or not (buf[c.offset + n:].cpu().numpy() == Cs.POISON).all():
        bad.append("%s: the source's surroundings changed" % c.name)
    return bad


def _child(S, two):
    L = probe()
    bad = []
    for c in Cs.built(S):
        bad += search(L, c, S, two=two)
    for b in bad:
        print("BAD " + b)
    print("CHILD ran %d cases" % len(Cs.built(S)))
    sys.exit(1 if bad else 0)


def test_segment_sizes():
    L = probe()
    got = [L.nxz_blockfind_segment(n) for n in (1 << 20, (1 << 20) + 1, 2 << 20, (2 << 20) + 1, 8 << 20, (8 << 20) + 1)]
    assert got == [1024, 2048, 2048, 4096, 4096, 8192]
    assert got == [M.segment_bytes(n) for n in (1 << 20, (1 << 20) + 1, 2 << 20, (2 << 20) + 1, 8 << 20, (8 << 20) + 1)]


def test_block_search_at_the_default_settings():
    assert not any(os.environ.get(k) for k in ("NXZ_BLOCKFIND_SEG", "NXZ_BLOCKFIND_TWO", "NXZ_BLOCKFIND_DIAG"))
    L = probe()
    bad = []
    for c in Cs.built(1024):
        bad += search(L, c, 1024)
    assert not bad, "\n".join(bad[:40])


def test_block_search_at_other_settings_in_child_processes():
    """segments of 512, 2048 and 8192 bytes (the overflow -- more passers than the first kernel hands over -- and the passes of
    8192 positions need 2 KiB at least), and the first kernel alone: a process each, one at a time, the first that fails ends it"""
    for S, two in ((512, True), (2048, True), (8192, True), (1024, False)):
        env = {k: v for k, v in os.environ.items() if not k.startswith("NXZ_BLOCKFIND_")}
        if S != 1024:
            env["NXZ_BLOCKFIND_SEG"] = str(S)
        if not two:
            env["NXZ_BLOCKFIND_TWO"] = "0"
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(S), str(int(two))], env=env, capture_output=True, text=True, timeout=300)
        assert p.returncode == 0 and "CHILD ran" in p.stdout, (S, two, p.returncode, p.stdout[-3000:], p.stderr[-2000:])


def handmade_stream():
    """-> (stream, the bits at which its dynamic blocks start): fourteen dynamic blocks of 1 KiB of output each (three tables), a run
    of three stored blocks in the middle, a fixed block, and a final dynamic block"""
    w = H.Bits()
    starts = []
    tables = [(H.GEN_LL, H.GEN_DD, {}), (Cs.LL16, Cs.DD16, {"syms": H.with_runs(Cs.LL16 + Cs.DD16, [(284, 16, 5)])}),
              (Cs.RUNS_LL, H.GEN_DD, {"syms": H.with_runs(Cs.RUNS_LL + H.GEN_DD, [(0, 18, 138)])})]
    rng = np.random.default_rng(17)

    def dyn(k, final=0):
        ll, dd, kw = tables[k % 3]
        starts.append(w.n)
        c = H.dynamic(w, final, ll, dd, **kw)
        lo = 138 if ll is Cs.RUNS_LL else 0
        c.lits(bytes(rng.integers(lo, 256, 1000, dtype=np.uint8)))
        c.match(24, 100 + k)
        c.eob()

    for k in range(7):
        dyn(k)
    for k in range(3):
        H.stored(w, bytes(rng.integers(0, 256, 300 + k, dtype=np.uint8)))
    for k in range(7, 11):
        dyn(k)
    c = H.fixed(w); c.lits(b"a fixed block between dynamic ones " * 8); c.match(258, 35); c.eob()
    for k in range(11, 14):
        dyn(k)
    dyn(14, final=1)
    return w.data(), starts


def test_hand_built_blocks_through_inflate_stream():
    """rc 0, bytes, CRC-32 and Adler-32 against zlib.  Pieces: the search finds every dynamic block's start (asserted against the
    model here), and the decode makes at least as many pieces as the model's `first` entries that are true block starts behind a
    dynamic block (a start behind the stored run or the fixed block may be decoded as part of the piece in front; nxz_pinflate.cpp
    adds token boundaries inside blocks on top: 25 pieces for 12 such starts when this was written)."""
    import torch
    pkg = importlib.import_module("power-gzip_amd")
    comp, starts = handmade_stream()
    plain = zlib.decompress(comp, -15)
    assert len(comp) >= 12 << 10 and len(plain) > 15000
    e = M.expected(comp, 0, M.segment_bytes(len(comp)))
    found = set(e.first) | set(x for m in e.more for x in m)
    assert all(M.Scan(comp).passes(b, 8 * len(comp)) for b in starts[:3]) and len(found & set(starts)) >= 10
    eng = pkg.Engine(0)
    try:
        src = torch.from_numpy(np.frombuffer(comp, np.uint8).copy()).to(eng.dev)
        dst = torch.zeros(len(plain) + 4096, dtype=torch.uint8, device=eng.dev)
        rc, info = eng.inflate_stream(src, len(comp), dst)
        torch.cuda.synchronize()
        print("pieces", info.get("pieces"), "rounds", info.get("rounds"), "block starts the model finds", len(found & set(starts)))
        assert rc == 0, (rc, info)
        assert info["out_len"] == len(plain) and info["crc"] == zlib.crc32(plain) and info["adler"] == zlib.adler32(plain)
        assert dst[:len(plain)].cpu().numpy().tobytes() == plain
        assert (dst[len(plain):] == 0).all()
        behind_dynamic = [b for i, b in enumerate(starts) if i not in (0, 7, 11)]          # (7: behind the stored run, 11: behind the fixed block)
        assert info["pieces"] >= max(3, len(set(e.first) & set(behind_dynamic))) and (info["end_bit"] + 7) // 8 == len(comp)
    finally:
        eng.close()


if __name__ == "__main__" and sys.argv[1:2] == ["--child"]:
    _child(int(sys.argv[2]), bool(int(sys.argv[3])))
