"""GPU tests of BGZF random access (include/nxz_engine.h: nxz_bgzf_index, nxz_bgzf_read_ranges; kernels in
power-gzip_amd/csrc/nxz_bgzf.hip): the index against a Python walk of the members (tests/bgzf_model.py), ranges in uncompressed
and in virtual offsets against slices of gzip.decompress, index slices, stale indexes, damaged members, the one-decode-per-member
rule, -E2BIG, chunked decodes, and the nxz_gzip options -i / -r / -b / -s."""
import ctypes as C
import errno
import gzip
import importlib
import os
import random
import subprocess

import numpy as np
import pytest

import bgzf_model as M
from datagen import make_block

pytestmark = pytest.mark.gpu
pkg = importlib.import_module("power-gzip_amd")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "power-gzip_amd", "nxz_gzip")
KNOBS = ("NXZ_INFLATE_LANES_MIN", "NXZ_INFLATE_CUT", "NXZ_INFLATE_WG", "NXZ_INFLATE_WG_MAX", "NXZ_WG_PMIN", "NXZ_INFLATE_ORDER",
         "NXZ_BGZF_CHUNK")
SINK = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t)


class BlockedOpts(C.Structure):
    _fields_ = [("device", C.c_int), ("fixed", C.c_int), ("block_size", C.c_uint32), ("chunk_blocks", C.c_uint32),
                ("group", C.c_uint32), ("reserved", C.c_uint32 * 3)]


@pytest.fixture(scope="module")
def eng():
    saved = {k: os.environ.pop(k, None) for k in KNOBS}
    e = pkg.Engine(0)
    yield e
    e.close()
    for k, v in saved.items():
        if v is not None:
            os.environ[k] = v


def blocked_image(data):
    """nxz_blocked_deflate's members of data (packed on the device by nxz_batch_pack_gzip), then the end marker"""
    L = C.CDLL(os.path.join(ROOT, "power-gzip_amd", "libnxz_amd.so"))
    L.nxz_blocked_deflate.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(BlockedOpts), SINK, C.c_void_p, C.POINTER(C.c_uint64)]
    parts = []
    sink = SINK(lambda u, b, n: parts.append(C.string_at(b, n)) or 0)
    assert L.nxz_blocked_deflate(data, len(data), C.byref(BlockedOpts(device=0)), sink, None, None) == 0
    return b"".join(parts) + M.EOF_MARKER


def corpus(n, seed=0):
    kinds = ["alice", "lz", "text33", "random", "zeros"]
    out, i = [], 0
    while sum(map(len, out)) < n:
        out.append(make_block(kinds[i % 5], 65536, seed=seed + i))
        i += 1
    return b"".join(out)[:n]


def odd_image(rnd, data):
    """a Python-built BGZF: members of odd sizes and levels, empty members (runs of them too), other extra subfields, end marker"""
    parts, pos = [], 0
    while pos < len(data):
        r = rnd.random()
        if r < 0.08:
            parts += [M.member(b"")] * rnd.randrange(1, 4)
            continue
        n = min(len(data) - pos, rnd.choice([1, 7, 4095, 65280, rnd.randrange(1, 65281)]))
        extra = (b"XY\x03\x00abc", b"") if r < 0.2 else (b"", b"ZZ\x01\x00q") if r < 0.3 else (b"", b"")
        parts.append(M.member(data[pos:pos + n], rnd.choice([0, 1, 6, 9]), *extra))
        pos += n
    return b"".join(parts) + M.EOF_MARKER


def dev(eng, b, pad_front=0):
    import torch
    h = np.zeros(pad_front + len(b) + 16, np.uint8)
    h[pad_front:pad_front + len(b)] = np.frombuffer(b, np.uint8)
    t = torch.from_numpy(h).to(eng.dev)
    return t[pad_front:]


def index(eng, image, max_members=None):
    t = dev(eng, image)
    mm = max_members or len(image) // 28 + 2
    coff, uoff = eng.bgzf_index(t, len(image), mm)
    return t, coff, uoff


def read(eng, t, length, coff, uoff, ranges, kind=M.UOFF, dst=None):
    import torch
    r = torch.tensor(np.array(ranges, np.uint64).reshape(-1, 2).view(np.int64), device=eng.dev)
    rc, offs, st, out_len, decoded, dst = eng.bgzf_read_ranges(t, length, coff, uoff, r, kind, dst)
    torch.cuda.synchronize(eng.dev)
    return rc, offs.cpu().numpy(), st.cpu().numpy(), out_len, decoded, dst


def check(plain, ranges_u, offs, st, dst, damaged=()):
    out = dst.cpu().numpy()[:offs[-1]].tobytes() if offs[-1] else b""
    for i, (b, e) in enumerate(ranges_u):
        if i in damaged:
            assert st[i] == M.DAMAGED and out[offs[i]:offs[i + 1]] == bytes(offs[i + 1] - offs[i]), i
        else:
            assert st[i] == M.OK and offs[i + 1] - offs[i] == e - b and out[offs[i]:offs[i + 1]] == plain[b:e], (i, b, e)


@pytest.fixture(scope="module")
def big(eng):
    data = corpus(12 << 20, seed=3)
    img = blocked_image(data)
    t, coff, uoff = index(eng, img)
    return data, img, t, coff.cpu().tolist(), uoff.cpu().tolist(), coff, uoff


def test_index_equals_a_walk_of_the_members(eng, big):
    data, img, _, coff, uoff, _, _ = big
    assert (coff, uoff) == M.index(img) and uoff[-1] == len(data) and coff[-1] == len(img)
    rnd = random.Random(2)
    odd = odd_image(rnd, corpus(3 << 20, seed=9))
    _, c, u = index(eng, odd)
    assert (c.cpu().tolist(), u.cpu().tolist()) == M.index(odd)
    # a member-like pattern inside a payload (stored, so the bytes stand there as they are) is no member
    fake = M.member(b"fake member " * 100)
    img2 = M.member(b"a" * 100) + M.member(b"x" * 50 + fake + b"y" * 50, 0) + M.member(b"z" * 100) + M.EOF_MARKER
    assert img2.find(fake, 30) > 0
    _, c, u = index(eng, img2)
    assert (c.cpu().tolist(), u.cpu().tolist()) == M.index(img2) and len(c) == 5
    # errors: no member at 0; more members than allowed
    with pytest.raises(pkg.EngineError):
        index(eng, b"\0" + img2)
    with pytest.raises(pkg.EngineError):
        index(eng, img2, max_members=2)


def test_random_uoff_ranges_equal_slices(eng, big):
    data, img, t, coff, uoff, dc, du = big
    assert gzip.decompress(img) == data
    rnd = random.Random(4)
    U = len(data)
    ranges = []
    for _ in range(3000):
        n = int(2 ** rnd.uniform(0, 20))
        b = rnd.randrange(0, U - n + 1)
        ranges.append((b, b + n))
    ranges += [(u, min(U, u + 65280)) for u in uoff[1:30]] + [(max(0, u - 5), u) for u in uoff[1:30]]
    ranges += [(0, U), (0, 1), (U - 1, U), (U, U), (7, 7)]
    rc, offs, st, out_len, decoded, dst = read(eng, t, len(img), dc, du, ranges)
    assert rc == 0 and out_len == offs[-1] == sum(e - b for b, e in ranges)
    assert decoded == len(coff) - 2                     # every member but the (empty) end marker holds a byte of some range
    check(data, ranges, offs, st, dst)


def test_virtual_offsets(eng, big):
    data, img, t, coff, uoff, dc, du = big
    rnd = random.Random(6)
    ur, vr = [], []
    for _ in range(500):
        b = rnd.randrange(0, len(data))
        e = min(len(data), b + int(2 ** rnd.uniform(0, 18)))
        ur.append((b, e))
        vr.append((M.voff(coff, uoff, b), M.voff(coff, uoff, e, at_end=rnd.random() < 0.5)))
    ur.append((0, len(data)))
    vr.append((0, coff[-1] << 16))
    bad = [len(vr), len(vr) + 1]
    vr += [((coff[3] + 1) << 16, coff[5] << 16), (coff[3] << 16 | 65535, coff[5] << 16)]   # not a member start; within > ISIZE
    ur += [(0, 0), (0, 0)]
    rc, offs, st, _, _, dst = read(eng, t, len(img), dc, du, vr, kind=M.VOFF)
    assert rc == 0 and [st[i] for i in bad] == [M.BAD_VOFFSET] * 2 and offs[bad[0]] == offs[bad[1] + 1]
    check(data, ur[:bad[0]], offs, st, dst)


def test_index_slice_reads_the_same_bytes(eng, big):
    data, img, _, coff, uoff, dc, du = big
    i, k = 17, 60                                     # members 17 .. 76
    sub = img[coff[i]:coff[i + k]]
    ts = dev(eng, sub, pad_front=5)                   # (any alignment of the sub-image)
    rnd = random.Random(8)
    ranges = [(uoff[i], uoff[i + k]), (uoff[i], uoff[i] + 1), (uoff[i + k] - 1, uoff[i + k])]
    for _ in range(100):
        b = rnd.randrange(uoff[i], uoff[i + k])
        ranges.append((b, rnd.randrange(b, uoff[i + k] + 1)))
    rc, offs, st, _, _, dst = read(eng, ts, len(sub), dc[i:i + k + 1], du[i:i + k + 1], ranges)
    assert rc == 0
    check(data, ranges, offs, st, dst)
    rc2, offs2, st2, _, _, dst2 = read(eng, big[2], len(img), dc, du, ranges)
    assert rc2 == 0 and (offs2 == offs).all() and (dst2.cpu().numpy()[:offs[-1]] == dst.cpu().numpy()[:offs[-1]]).all()
    # outside the slice: out of bounds
    rc, offs, st, _, _, _ = read(eng, ts, len(sub), dc[i:i + k + 1], du[i:i + k + 1], [(uoff[i] - 1, uoff[i] + 5), (uoff[i], uoff[i + k] + 1)])
    assert rc == 0 and st.tolist() == [M.OUT_OF_BOUNDS] * 2 and offs.tolist() == [0, 0, 0]


def test_stale_index_and_damaged_members(eng):
    import torch
    rnd = random.Random(10)
    data = corpus(2 << 20, seed=20)
    img = odd_image(rnd, data)
    other = odd_image(random.Random(11), data)
    t, dc, du = index(eng, img)
    _, oc, ou = index(eng, other)
    coff, uoff = dc.cpu().tolist(), du.cpu().tolist()
    ranges = [(0, len(data)), (5, 6)]
    moved = dc.clone()
    moved[len(coff) // 2] += 1
    for c, u in ((oc, ou), (dc[1:], du[1:]), (moved, du)):         # another image's index, shifted by a member, one start moved
        rc, _, _, _, _, _ = read(eng, t, len(img), c, u, ranges, dst=torch.zeros(len(data) + 16, dtype=torch.uint8, device=eng.dev))
        assert rc == -errno.EILSEQ
    # damage one member's deflate data: only the ranges that touch it are DAMAGED, and zeros
    j = next(j for j in range(5, len(coff) - 1) if uoff[j + 1] - uoff[j] > 1000 and coff[j + 1] - coff[j] > 200)
    bad = bytearray(img)
    mid = (coff[j] + coff[j + 1]) // 2
    bad[mid] ^= 0xff
    bad[mid + 1] ^= 0x55
    tb = dev(eng, bytes(bad))
    ranges = [(0, len(data)), (uoff[j], uoff[j] + 10), (uoff[j] - 3, uoff[j]), (uoff[j + 1], uoff[j + 1] + 100), (uoff[j + 1] - 1, uoff[j + 1] + 1)]
    ranges += [(b, b + 2000) for b in range(0, len(data) - 2000, 99991)]
    touch = {i for i, (b, e) in enumerate(ranges) if b < uoff[j + 1] and e > uoff[j]}
    dst = torch.full((sum(e - b for b, e in ranges) + 16,), 0xee, dtype=torch.uint8, device=eng.dev)
    rc, offs, st, _, _, dst = read(eng, tb, len(bad), dc, du, ranges, dst=dst)
    assert rc == 0 and touch and len(touch) < len(ranges)
    check(data, ranges, offs, st, dst, damaged=touch)


def test_each_member_is_decoded_once(eng, big):
    data, img, t, coff, uoff, dc, du = big
    b, e = uoff[3] + 100, uoff[9] + 5
    rc, _, _, _, one, _ = read(eng, t, len(img), dc, du, [(b, e)])
    rc2, offs, st, _, many, dst = read(eng, t, len(img), dc, du, [(b, e)] * 500 + [(b + 1, e - 1)] * 100)
    assert rc == rc2 == 0 and one == many == 7
    check(data, [(b, e)] * 500 + [(b + 1, e - 1)] * 100, offs, st, dst)


def test_too_small_a_destination(eng, big):
    import torch
    data, img, t, coff, uoff, dc, du = big
    ranges = [(10, 5000), (70000, 300000), (5, 5)]
    need = sum(e - b for b, e in ranges)
    rc, offs, st, out_len, decoded, _ = read(eng, t, len(img), dc, du, ranges, dst=torch.zeros(need - 1, dtype=torch.uint8, device=eng.dev))
    assert rc == -errno.E2BIG and out_len == need and decoded == 0
    rc, offs, st, out_len, _, dst = read(eng, t, len(img), dc, du, ranges, dst=torch.zeros(need, dtype=torch.uint8, device=eng.dev))
    assert rc == 0 and out_len == need
    check(data, ranges, offs, st, dst)


def test_chunked_decode_gives_the_same_bytes(eng):
    rnd = random.Random(12)
    data = corpus(4 << 20, seed=40)
    parts = []
    for p in range(0, len(data), 4096):               # ~1 000 members
        parts.append(M.member(data[p:p + 4096], 1))
    img = b"".join(parts) + M.EOF_MARKER
    t, dc, du = index(eng, img)
    assert len(dc) > 1000
    ranges = [(0, len(data))] + [(b, min(len(data), b + rnd.randrange(1, 300000))) for b in (rnd.randrange(len(data)) for _ in range(300))]
    rc, offs, st, _, d1, dst = read(eng, t, len(img), dc, du, ranges)
    assert rc == 0
    check(data, ranges, offs, st, dst)
    os.environ["NXZ_BGZF_CHUNK"] = "64"
    try:
        rc, offs2, st2, _, d2, dst2 = read(eng, t, len(img), dc, du, ranges)
    finally:
        del os.environ["NXZ_BGZF_CHUNK"]
    assert rc == 0 and d1 == d2 == len(dc) - 2
    assert (offs2 == offs).all() and (dst2.cpu().numpy()[:offs[-1]] == dst.cpu().numpy()[:offs[-1]]).all()


def test_cli_index_and_ranges(tmp_path):
    data = corpus(3 << 20, seed=50)
    src = tmp_path / "f"
    src.write_bytes(data)
    run = lambda *a: subprocess.run([CLI] + [str(x) for x in a], capture_output=True, timeout=300)
    r = run("-k", "-i", src)
    assert r.returncode == 0, r.stderr
    gz, gzi = tmp_path / "f.gz", tmp_path / "f.gz.gzi"
    img = gz.read_bytes()
    assert gzip.decompress(img) == data
    want = M.gzi_bytes(*M.index(img))
    assert gzi.read_bytes() == want
    gzi.unlink()
    r = run("-r", gz)
    assert r.returncode == 0, r.stderr
    assert gzi.read_bytes() == want
    other = tmp_path / "other.gzi"
    assert run("-r", "-I", other, gz).returncode == 0 and other.read_bytes() == want
    cases = [(0, 1), (65279, 2), (1000000, 500000), (len(data) - 1, 1), (0, len(data)), (12345, 0)]
    for with_index in (True, False):
        if not with_index:
            gzi.unlink()
        for b, n in cases:
            r = run("-d", "-c", "-b", b, "-s", n, gz)
            assert r.returncode == 0 and r.stdout == data[b:b + n], (with_index, b, n, r.stderr)
        r = run("-d", "-c", "-b", len(data) - 10, gz)           # no -s: to the end
        assert r.returncode == 0 and r.stdout == data[-10:]
        assert run("-d", "-c", "-b", len(data) + 1, "-s", 1, gz).returncode != 0
    r = run("-d", "-c", "-b", 100, "-s", 50, "-I", other, gz)
    assert r.returncode == 0 and r.stdout == data[100:150]
