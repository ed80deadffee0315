"""GPU tests (-m gpu) of the kernels that move data between the rounds of the one-stream inflate (power-gzip_amd/csrc/
nxz_blockfind.hip: stored_walk_kernel, copy_items_kernel, differ_items_kernel, window_chain_kernel and compose_maps_kernel in
both forms, resolve_kernel), each called through its launcher in power-gzip_amd/libnxz_blockfind_probe.so -- the object file
the engine ships -- and compared with numpy or plain Python at the sizes and alignments where each takes another path.

The window chain has three launch shapes: one kernel (two groups of 8 pieces at most), two levels, and three levels above
NXZ_CHAIN_TWO_LEVELS_MAX groups (64: more than 512 pieces).  The launcher reads that setting once a process, so the third shape
runs in a child process with the setting at 2: 100 pieces (13 groups, one group of groups) and 259 (33 groups, three groups of
groups, the last of one group).  The buffers for the groups' maps and windows are sized by nxz_pinflate.cpp's own formula:
n / 8 + n / 128 + 4 maps of 64 KiB and as many windows of 32 KiB."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":                       # a child process: no conftest has set the path
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))

import deflate_handmade as H

pytestmark = pytest.mark.gpu
PROBE = os.path.join(ROOT, "power-gzip_amd", "libnxz_blockfind_probe.so")
WINDOW = 32768
_lib = None


def probe():
    global _lib
    if _lib is None:
        import torch  # (first: the library then shares torch's HIP runtime, as the engine does -- power-gzip_amd/engine.py)
        torch.cuda.init()
        L = C.CDLL(PROBE)
        P, U32 = C.c_void_p, C.c_uint32
        for name, args in (("nxz_launch_stored_walk", [P, U32, P, P]), ("nxz_launch_copy_items", [P, U32, P]),
                           ("nxz_launch_differ_items", [P, U32, P, P]), ("nxz_launch_window_chain", [P, U32, P, P, P, P, P]),
                           ("nxz_launch_resolve", [P, U32, P, P, P, P])):
            getattr(L, name).restype = C.c_int
            getattr(L, name).argtypes = args
        L.nxz_window_chain_group.restype = U32
        L.nxz_window_chain_group.argtypes = [U32]
        _lib = L
    return _lib


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


# ---- stored_walk ----------------------------------------------------------------------------------------------------------

WALK_REQ = np.dtype([("src", "<u8"), ("src_len", "<u8"), ("bit", "<u8"), ("rem", "<u4"), ("bfinal", "<u4")])
WALK_RES = np.dtype([("bit", "<u8"), ("flags", "<u4"), ("reserved", "<u4")])


def walk_ref(src, bit, rem, bfinal):
    """nxz_blockfind.hip's comment: from `rem` bytes inside a stored block to the header of the first block that is not a stored one
    -- or that is not whole inside the source, or whose LEN and NLEN do not match -- or to the end of a final stored block (flags 1)"""
    total, pos, fin = 8 * len(src), bit + 8 * rem, bfinal

    def b(p):
        return src[p >> 3] >> (p & 7) & 1
    while True:
        if fin:
            return pos, 1
        if pos + 3 > total or b(pos + 1) or b(pos + 2):
            return pos, 0
        p2 = (pos + 3 + 7) & ~7
        if p2 + 32 > total:
            return pos, 0
        q = p2 >> 3
        ln, nl = src[q] | src[q + 1] << 8, src[q + 2] | src[q + 3] << 8
        if ln ^ nl != 0xffff or p2 + 32 + 8 * ln > total:
            return pos, 0
        fin, pos = b(pos), p2 + 32 + 8 * ln


def walk_requests():
    """[(stream, bit, rem, bfinal)]"""
    rng = np.random.default_rng(23)
    out = []

    def blocks(off, lens, end, final_last=0):
        w = H.Bits()
        w.put(int(rng.integers(0, 1 << off)) if off else 0, off)
        for i, n in enumerate(lens):
            H.stored(w, bytes(rng.integers(0, 256, n, dtype=np.uint8)), final=final_last if i + 1 == len(lens) else 0)
        if end == "dynamic":
            w.put(0, 1); w.put(2, 2); w.put(0x155, 14)
            data = w.data() + bytes(rng.integers(0, 256, 9, dtype=np.uint8))
        elif end == "fixed":
            w.put(1, 1); w.put(1, 2)
            data = w.data() + bytes(rng.integers(0, 256, 9, dtype=np.uint8))
        elif end == "mismatch":
            H.stored(w, b"abc", nlen=0xfff0)
            data = w.data()
        elif end == "one-byte-beyond":
            H.stored(w, b"abcdefgh")
            data = w.data()[:-1]
        elif end == "fewer-than-32-bits":
            w.put(0, 3)
            data = w.data() + b"\x05\x00"
        else:                                              # "end": nothing behind the last block (fewer than 3 bits)
            data = w.data()
        return data

    for off in range(8):
        for lens, end in (([5], "dynamic"), ([3, 0], "fixed"), ([1] * 40, "dynamic"), ([7, 2], "mismatch"), ([4], "one-byte-beyond"),
                          ([6], "fewer-than-32-bits"), ([2, 9], "end")):
            out.append((blocks(off, lens, end), off, 0, 0))
        out.append((blocks(off, [3, 4], "fixed", final_last=1), off, 0, 0))             # ends at a final stored block: flags 1
    out.append((blocks(0, [0, 65535, 0, 12], "fixed"), 0, 0, 0))
    out.append((blocks(5, [65535], "end", final_last=1), 5, 0, 0))
    s = blocks(0, [100, 3], "dynamic")
    out.append((s, 8 * 45, 60, 0))                        # 60 bytes of the first block to come (5 bytes of header, 40 of data behind us)
    out.append((s, 8 * 105, 0, 0))
    out.append((s, 8 * 45, 60, 1))                        # ... of a final block: its end, flags 1
    out.append((blocks(6, [5], "fixed"), 6, 0, 1))        # bfinal set at a header: stays where it is, flags 1
    return out


@pytest.mark.parametrize("n", [1, 64, 65, None])
def test_stored_walk(n):
    import torch
    L = probe()
    reqs = walk_requests()[:n]
    assert n is None or len(reqs) == n
    blob, at = bytearray(), []
    for s, _, _, _ in reqs:
        at.append(len(blob))
        blob += s + b"\xa5" * (5 + len(s) % 3)            # (no zeros behind a stream, and streams at any alignment)
    src = dev(np.frombuffer(bytes(blob), np.uint8))
    rq = np.zeros(len(reqs), WALK_REQ)
    for i, (s, bit, rem, fin) in enumerate(reqs):
        rq[i] = (src.data_ptr() + at[i], len(s), bit, rem, fin)
    d_rq = dev(rq)
    GUARD = 4
    res = torch.full(((len(reqs) + 2 * GUARD) * 16,), 0x5a, dtype=torch.uint8, device="cuda")
    assert L.nxz_launch_stored_walk(d_rq.data_ptr(), len(reqs), res.data_ptr() + 16 * GUARD, None) == 0
    raw = host(res)
    got = raw[16 * GUARD:16 * (GUARD + len(reqs))].view(WALK_RES)
    assert (raw[:16 * GUARD] == 0x5a).all() and (raw[16 * (GUARD + len(reqs)):] == 0x5a).all()
    for i, (s, bit, rem, fin) in enumerate(reqs):
        assert (int(got["bit"][i]), int(got["flags"][i]), int(got["reserved"][i])) == walk_ref(s, bit, rem, fin) + (0,), (i, bit, rem, fin, len(s))
    if n is None:
        refs = [walk_ref(*r) for r in reqs]
        assert sum(f for _, f in refs) >= 10 and len(set(r[1] for r in reqs)) == 8 + 2


# ---- copy_items, differ_items ---------------------------------------------------------------------------------------------

ITEM = np.dtype([("src", "<u8"), ("dst", "<u8"), ("bytes", "<u8")])
SIZES = (0, 1, 15, 16, 63, 64, 65, 4099)
ALIGN = (0, 1, 8, 15)


def fill_ref(mode, n):
    k = np.arange(n, dtype=np.uint64)
    return (np.zeros(n, np.uint8) if mode == 0 else (k & 255).astype(np.uint8) if mode == 1 else ((k >> 8) & 255).astype(np.uint8) if mode == 2
            else (255 - (k & 255)).astype(np.uint8))


def test_copy_items():
    import torch
    L = probe()
    rng = np.random.default_rng(29)
    plan, s_at, d_at = [], 0, 64                            # (kind, source offset or fill mode, destination offset, bytes)
    for n in SIZES:
        for sa in ALIGN:
            for da in ALIGN:
                s_at = (s_at + 15) // 16 * 16 + sa
                d_at = (d_at + 15) // 16 * 16 + 32 + da     # (32 bytes of canary at least between two destinations)
                plan.append(("copy", s_at, d_at, n))
                s_at += n
                d_at += n
    for mode in range(4):
        for n, da in ((1, 3), (255, 0), (256, 15), (257, 8), (70000, 5)):                # (70000: k >> 8 goes past 255)
            d_at = (d_at + 15) // 16 * 16 + 32 + da
            plan.append(("fill", mode, d_at, n))
            d_at += n
    srcb = rng.integers(0, 256, s_at + 64, dtype=np.uint8)
    want = np.full(d_at + 64, 0xee, np.uint8)
    src, dst = dev(srcb), dev(want)
    assert src.data_ptr() % 16 == 0 and dst.data_ptr() % 16 == 0 and src.data_ptr() >= 16
    items = np.zeros(len(plan), ITEM)
    for i, (kind, a, d, n) in enumerate(plan):
        items[i] = (src.data_ptr() + a if kind == "copy" else a, dst.data_ptr() + d, n)
        want[d:d + n] = srcb[a:a + n] if kind == "copy" else fill_ref(a, n)
    d_items = dev(items)
    assert L.nxz_launch_copy_items(d_items.data_ptr(), len(plan), None) == 0
    got = host(dst)
    for kind, a, d, n in plan:
        assert (got[d - 32:d + n + 32] == want[d - 32:d + n + 32]).all(), (kind, a, d % 16, n)
    assert (got == want).all() and (host(src) == srcb).all()


@pytest.mark.parametrize("preset", [0, 0x5a5a5a5a])
def test_differ_items(preset):
    import torch
    L = probe()
    rng = np.random.default_rng(31)
    a = rng.integers(0, 256, 1 << 16, dtype=np.uint8)
    b = a.copy()
    plan, at = [], 0                                        # (offset in a, offset in b, bytes, differ)
    for n in (0, 1, 2, 255, 256, 257, 4099):
        for how in ("equal", "first", "last", "middle"):
            if how != "equal" and (n == 0 or (how == "middle" and n < 3)):
                continue
            oa, ob = at + 1, at + 16 + 7                    # (the two ranges at different alignments)
            b[ob:ob + n] = a[oa:oa + n]
            if how != "equal":
                b[ob + {"first": 0, "last": n - 1, "middle": n // 2}[how]] ^= 0x10
            plan.append((oa, ob, n, how != "equal"))
            at = ob + n + 16
    assert at < len(a)
    da, db = dev(a), dev(b)
    items = np.zeros(len(plan), ITEM)
    for i, (oa, ob, n, _) in enumerate(plan):
        items[i] = (da.data_ptr() + oa, db.data_ptr() + ob, n)
    d_items = dev(items)
    flags = torch.from_numpy(np.full(len(plan) + 8, preset, np.uint32).view(np.int32)).cuda()
    assert L.nxz_launch_differ_items(d_items.data_ptr(), len(plan), flags.data_ptr() + 16, None) == 0
    got = host(flags).view(np.uint32)
    want = np.full(len(plan) + 8, preset, np.uint32)
    want[4:4 + len(plan)][[p[3] for p in plan]] = 1         # (the kernel writes a 1 and nothing else)
    assert (got == want).all(), (got, want)
    assert (host(da) == a).all() and (host(db) == b).all()


# ---- window_chain, resolve ------------------------------------------------------------------------------------------------

PIECE = np.dtype([("o", "<u8"), ("len", "<u8"), ("place", "<u8")])
EDGE_LENGTHS = (0, 1, 7, 8, 9, 32767, 32768, 32769, 65536 + 5, 140000)


def chain_case(lengths, seed):
    """pieces of 16-bit elements, about half of them bytes and half 0x8000 | index over all of 0..32767 -> (elements with the pieces
    at even byte offsets that are no multiples of 16, their offsets, places that run through all four values mod 4, win0, the
    windows behind every piece, the resolved target with 0xc3 between the pieces and behind the last)"""
    rng = np.random.default_rng(seed)
    win0 = rng.integers(0, 256, WINDOW, dtype=np.uint8)
    els, offs, places, at, place = [], [], [], 0, 8
    for i, n in enumerate(lengths):
        e = np.where(rng.integers(0, 2, n).astype(bool), 0x8000 | rng.integers(0, 32768, n), rng.integers(0, 256, n)).astype(np.uint16)
        if n:
            e[-1] = 0x8000 | (0, 32767)[i % 2]
        at = (at + 15) // 16 * 16 + (2, 6, 10, 14)[i % 4]
        offs.append(at)
        els.append(e)
        at += 2 * n
        place += (3 * i - place) % 4                        # (place mod 4: 0, 3, 2, 1, ...)
        places.append(place)
        place += n + 5                                      # (5 to 8 bytes of canary between two pieces)
    assert set(p % 4 for p in places) == set(range(4)) or len(lengths) < 4
    blob = np.full(at + 64, 0x77, np.uint8)
    for o, e in zip(offs, els):
        blob[o:o + 2 * len(e)] = e.view(np.uint8)
    dst = np.full(place + 64, 0xc3, np.uint8)
    windows = np.zeros((len(lengths), WINDOW), np.uint8)
    win = win0
    for i, e in enumerate(els):
        out = np.where(e & 0x8000, win[e & 0x7fff], e & 0xff).astype(np.uint8)
        dst[places[i]:places[i] + len(e)] = out
        win = np.concatenate([win, out])[-WINDOW:]
        windows[i] = win
    return blob, offs, places, win0, windows, dst


def run_chain(lengths, seed):
    import torch
    L = probe()
    n = len(lengths)
    blob, offs, places, win0, windows, dst = chain_case(lengths, seed)
    d_blob, d_win0 = dev(blob), dev(win0)
    pc = np.zeros(n, PIECE)
    for i in range(n):
        pc[i] = (d_blob.data_ptr() + offs[i], lengths[i], places[i])
    d_pc = dev(pc)
    assert L.nxz_window_chain_group(0) == 8
    ng0 = n // 8 + n // 128 + 4                            # nxz_pinflate.cpp: groups of the smallest size, and the groups of 16 of them
    d_windows = torch.full((n * WINDOW + 64,), 0x5a, dtype=torch.uint8, device="cuda")
    d_gmaps = torch.full((ng0 * WINDOW * 2 + 64,), 0x5a, dtype=torch.uint8, device="cuda")
    d_gwin = torch.full((ng0 * WINDOW + 64,), 0x5a, dtype=torch.uint8, device="cuda")
    d_dst = torch.full((len(dst),), 0xc3, dtype=torch.uint8, device="cuda")
    assert all(t.data_ptr() % 16 == 0 for t in (d_win0, d_windows, d_gmaps, d_gwin))
    assert L.nxz_launch_window_chain(d_pc.data_ptr(), n, d_win0.data_ptr(), d_windows.data_ptr(), d_gmaps.data_ptr(), d_gwin.data_ptr(), None) == 0
    assert L.nxz_launch_resolve(d_pc.data_ptr(), n, d_win0.data_ptr(), d_windows.data_ptr(), d_dst.data_ptr(), None) == 0
    w = host(d_windows)
    for i in range(n):
        assert (w[i * WINDOW:(i + 1) * WINDOW] == windows[i]).all(), ("the window behind piece", i, "of", n)
    assert (w[n * WINDOW:] == 0x5a).all() and (host(d_gmaps)[-64:] == 0x5a).all() and (host(d_gwin)[-64:] == 0x5a).all()
    got = host(d_dst)
    for i in range(n):
        a, b = places[i], places[i] + lengths[i]
        assert (got[a:b] == dst[a:b]).all(), ("piece", i, "of", n, "place", a, "length", lengths[i])
    assert (got == dst).all()                              # (the canaries between the pieces and behind the last)
    assert (host(d_blob) == blob).all() and (host(d_win0) == win0).all()


def many(n):
    return [(1, 300, 40000, 9, 33000)[i % 5] for i in range(n)]


@pytest.mark.parametrize("n", [1, 8, 16])
def test_window_chain_and_resolve_one_kernel(n):
    run_chain(many(n), n)


def test_window_chain_and_resolve_at_the_edge_lengths():
    """one kernel (10 pieces: two groups); 140000 elements are more than four chunks of 32 Ki, so that resolve's workgroups take a
    second chunk"""
    run_chain(list(EDGE_LENGTHS), 41)
    run_chain(list(EDGE_LENGTHS[::-1]), 42)


@pytest.mark.parametrize("n", [17, 100, 259])
def test_window_chain_and_resolve_two_levels(n):
    assert not os.environ.get("NXZ_CHAIN_GROUP") and not os.environ.get("NXZ_CHAIN_TWO_LEVELS_MAX")
    run_chain(many(n), n)


def test_window_chain_three_levels_in_a_child_process():
    env = {k: v for k, v in os.environ.items() if not k.startswith("NXZ_CHAIN_")}
    env["NXZ_CHAIN_TWO_LEVELS_MAX"] = "2"
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--chain-child"], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "CHILD ran" in p.stdout, (p.returncode, p.stdout[-3000:], p.stderr[-3000:])


if __name__ == "__main__" and sys.argv[1:] == ["--chain-child"]:
    assert os.environ.get("NXZ_CHAIN_TWO_LEVELS_MAX") == "2"
    for n in (100, 259):                                   # 13 groups and one group of groups; 33 groups and three, the last of one
        run_chain(many(n), n)
    print("CHILD ran")
