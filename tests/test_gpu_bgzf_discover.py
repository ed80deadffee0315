"""GPU tests (-m gpu) of the BGZF member discovery, called directly: nxz_bgzf_workspace, nxz_launch_bgzf_discover and
nxz_launch_bgzf_coff from power-gzip_amd/libnxz_frame_probe.so -- the object file the engine ships, linked without the engine's
version script -- over every hand-built image of tests/bgzf_discover_cases.py at its cap and max_members, compared with
tests/bgzf_model.py discover(): ctl, the candidate list, offsets, the members' jobs as addresses, coff.  The workspace, offsets,
coff and dst are filled with a sentinel and have 256 guard bytes behind them: what the model calls unwritten is compared byte
by byte with the sentinel, the guards and the image's surroundings always.

Then the decodable images through the public calls (Engine.unpack_gzip, Engine.bgzf_index) at three placements, and one image
with more false candidates than the first pass of the engine's discovery has room for, so that its second pass decides."""
import ctypes as C
import errno
import importlib
import os

import numpy as np
import pytest

import bgzf_discover_cases as Cs
import bgzf_model as M

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE = os.path.join(ROOT, "power-gzip_amd", "libnxz_frame_probe.so")
GUARD = 256
TILE = 16384


def up256(n):
    return (n + 255) & ~255


def probe():
    import torch  # noqa: F401  (first: the library then shares torch's HIP runtime, as the engine does -- power-gzip_amd/engine.py)
    torch.cuda.init()
    L = C.CDLL(PROBE)
    L.nxz_bgzf_workspace.restype = C.c_size_t
    L.nxz_bgzf_workspace.argtypes = [C.c_uint64, C.c_uint64]
    L.nxz_launch_bgzf_discover.restype = C.c_int
    L.nxz_launch_bgzf_discover.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64,
                                           C.POINTER(C.c_void_p), C.c_void_p]
    L.nxz_launch_bgzf_coff.restype = C.c_int
    L.nxz_launch_bgzf_coff.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p]
    return L


def place(c, head, dev="cuda"):
    """-> (tensor, offset of packed[0] in it, the host copy): the image at byte `head` of a granule with the case's surroundings"""
    import torch
    n = len(c.image)
    host = np.full(up256(head + Cs.PAD + n + Cs.PAD), 0xee, np.uint8)
    host[head:head + Cs.PAD + n + Cs.PAD] = np.frombuffer(c.before + c.image + c.after, np.uint8)
    t = torch.from_numpy(host).to(dev)
    assert t.data_ptr() % 16 == 0
    return t, head + Cs.PAD, host


def discover(L, c):
    """-> what is wrong with what the launchers leave for case c, a line each"""
    import torch
    n, cap, mm = len(c.image), c.cap, c.max_members
    src, at, host = place(c, c.head)
    packed = src.data_ptr() + at
    wsn = L.nxz_bgzf_workspace(n, cap)
    ws = torch.full((wsn + GUARD,), Cs.SENTINEL, dtype=torch.uint8, device="cuda")
    offsets = torch.full(((mm + 1) * 8 + GUARD,), Cs.SENTINEL, dtype=torch.uint8, device="cuda")
    coff = torch.full(((mm + 1) * 8 + GUARD,), Cs.SENTINEL, dtype=torch.uint8, device="cuda")
    dst = torch.full((2 * GUARD,), Cs.SENTINEL, dtype=torch.uint8, device="cuda")
    jobs = C.c_void_p()
    rc = L.nxz_launch_bgzf_discover(packed, n, dst.data_ptr(), offsets.data_ptr(), mm, ws.data_ptr(), cap, C.byref(jobs), None)
    rc2 = L.nxz_launch_bgzf_coff(packed, n, ws.data_ptr(), cap, mm, coff.data_ptr(), None)
    torch.cuda.synchronize()
    assert rc == 0 and rc2 == 0, (c.name, rc, rc2)
    w, o, co = ws.cpu().numpy(), offsets.cpu().numpy(), coff.cpu().numpy()
    # the workspace as the launcher lays it out: ctl, the tiles' counts and offsets, pos, size ...; the jobs where it says they are
    tiles = (n + c.head + TILE - 1) // TILE
    p = 256 + 2 * up256(tiles * 4 + 4)
    j = jobs.value - ws.data_ptr()
    assert p + up256(cap * 8) + up256(cap * 4) <= j and j + cap * Cs.JOB_DTYPE.itemsize <= wsn, (c.name, j, wsn)
    got = {"ctl": w[:32].view("<u8"), "pos": w[p:p + cap * 8].view("<u8"), "size": w[p + up256(cap * 8):][:cap * 4].view("<u4"),
           "offsets": o[:(mm + 1) * 8].view("<u8"), "coff": co[:(mm + 1) * 8].view("<u8"),
           "jobs": w[j:j + cap * Cs.JOB_DTYPE.itemsize].view(Cs.JOB_DTYPE), "packed": packed, "dst": dst.data_ptr(),
           "guards": {"the workspace": (w[wsn:] == Cs.SENTINEL).all(), "offsets": (o[(mm + 1) * 8:] == Cs.SENTINEL).all(),
                      "coff": (co[(mm + 1) * 8:] == Cs.SENTINEL).all(), "dst": bool((dst == Cs.SENTINEL).all()),
                      "the image (it changed)": (src.cpu().numpy() == host).all()}}
    return Cs.check(c, got)


def test_discovery_of_every_case():
    L = probe()
    bad, ran = [], dict.fromkeys(Cs.FAMILIES, 0)
    for c in Cs.cases():
        bad += discover(L, c)
        ran[c.family] += 1
    assert ran == {f: len(v) for f, v in Cs.by_family().items()} and all(ran.values())
    assert not bad, "\n".join(bad[:40])


def test_the_tile_images_have_two_and_three_tiles_a_lane():
    for c, tiles in zip(Cs.by_family()["tiles"], (1025, 2049)):
        assert (len(c.image) + c.head + TILE - 1) // TILE == tiles and c.model().L > 250 and c.model().ctl[0] > c.model().L + 200


@pytest.fixture(scope="module")
def eng():
    pkg = importlib.import_module("power-gzip_amd")
    e = pkg.Engine(0)
    yield e
    e.close()


def unpack_and_index(eng, c, head, max_members=None):
    """the image of c at byte `head` of a granule through both public calls, against the model's index and zlib's bytes"""
    import torch
    pkg = importlib.import_module("power-gzip_amd")
    coff, uoff = M.index(c.image)
    L, total = len(coff) - 1, uoff[-1]
    assert L > 0
    mm = L + 2 if max_members is None else max_members
    t, at, _ = place(c, head, eng.dev)
    packed = t[at:]
    dst = torch.full((total + 64,), 0xcd, dtype=torch.uint8, device=eng.dev)
    rc, d = eng.unpack_gzip(packed, len(c.image), dst, mm)
    torch.cuda.synchronize(eng.dev)
    if L > mm:
        assert rc == -errno.E2BIG and d["members"] == L and d["consumed"] == coff[-1], (c.name, head, rc, d["members"])
        with pytest.raises(pkg.EngineError):
            eng.bgzf_index(packed, len(c.image), mm)
        return
    assert rc == 0 and (d["members"], d["consumed"], d["out_len"]) == (L, coff[-1], total), (c.name, head, rc, d["members"], d["consumed"], d["out_len"])
    out = dst.cpu().numpy()
    assert out[:total].tobytes() == b"".join(Cs.plains(c)) and (out[total:] == 0xcd).all(), (c.name, head)
    assert d["offsets"].cpu().numpy()[:L + 1].tolist() == uoff, (c.name, head)
    gc, gu = eng.bgzf_index(packed, len(c.image), mm)
    assert gc.cpu().numpy().tolist() == coff and gu.cpu().numpy().tolist() == uoff, (c.name, head)


def test_decodable_cases_through_the_public_calls(eng):
    seen, ran, left_out = set(), dict.fromkeys(Cs.FAMILIES, 0), dict.fromkeys(Cs.FAMILIES, 0)
    for c in Cs.cases():
        if not c.decodable or c.device_only or (c.image in seen and c._mm is None):
            left_out[c.family] += 1                  # (not decodable, the megabytes of the tile images, or the same image once more)
            continue
        seen.add(c.image)
        for head in (0, 3, 15):
            unpack_and_index(eng, c, head, c._mm)
        ran[c.family] += 1
    assert all(ran[f] + left_out[f] == len(v) for f, v in Cs.by_family().items())
    assert all(ran[f] for f in Cs.FAMILIES if f != "tiles") and sum(ran.values()) > 100


def test_second_pass_of_the_engines_discovery():
    """over 3000 false candidates in one stored payload, four true members, max_members 4: the engine's first pass has room for
    max(2 * 4 + 1024, len / 32768 + 1024) = 1032 candidates, so the answer is the second pass's.  A fresh engine: one that has
    seen a larger image keeps its larger workspace"""
    pkg = importlib.import_module("power-gzip_amd")
    c = next(c for c in Cs.cases() if c.name == "limits-second-pass-every-candidate")
    assert c.model().ctl[0] > 3000 > max(2 * 4 + 1024, len(c.image) // 32768 + 1024) and c.model().L == 4
    e = pkg.Engine(0)
    try:
        for head in (3, 0, 15):
            unpack_and_index(e, c, head, 4)
    finally:
        e.close()
