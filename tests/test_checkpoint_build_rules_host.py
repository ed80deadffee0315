"""The rules of the one-pass index build (power-gzip_amd/csrc/nxz_checkpoint_build.h) -- the code the kernel of
nxz_checkpoint_build.hip runs -- compiled for the host under AddressSanitizer and UBSan (tests/native/checkpoint_build_host.cpp) and
held against plain Python: where an output byte lives in the ring, the pieces of a run and of a dump around the wrap, the source of
a match's bytes, and a ring driven through those rules against a bytearray.  The hand-built streams of the GPU test are checked
here too (tests/checkpoint_build_cases.py asserts what they must contain)."""
import os
import random
import subprocess

import pytest

import checkpoint_build_cases as B
import checkpoint_fine_model as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W = 32768
US = [0, 1, 32767, 32768, 32769, 65535, 65536, 65537, (1 << 32) - 1]


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    exe = tmp_path_factory.mktemp("cpb") / "checkpoint_build_host"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "power-gzip_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "checkpoint_build_host.cpp"), "-o", str(exe)], check=True)

    def run(lines):
        r = subprocess.run([str(exe)], input=("\n".join(lines) + "\n").encode(), capture_output=True, timeout=600)
        assert r.returncode == 0, (r.returncode, r.stderr.decode()[-4000:])
        out = r.stdout.decode().splitlines()
        assert len(out) == len(lines)
        return [[int(x) for x in line.split()] for line in out]
    return run


def pieces(u, n):
    s = u % W
    first = min(n, W - s)
    return [s, first, 0, n - first]


def test_ring_positions_and_dump_geometry(host):
    assert host(["pos %d" % u for u in US]) == [[u % W] for u in US]
    got = host(["dump %d" % u for u in US])
    for u, g in zip(US, got):
        w = min(u, W)
        assert g == pieces(u - w, w), u
        assert g[1] + g[3] == w and g[0] + g[1] <= W
    assert got[0] == [0, 0, 0, 0] and got[2] == [0, 32767, 0, 0] and got[3] == [0, 32768, 0, 0] and got[4] == [1, 32767, 0, 1]
    assert got[-1] == [32767, 1, 0, 32767]


def test_runs_on_both_sides_of_the_wrap(host):
    cases = [(u, n) for u in US + [32768 - 258, 32768 - 3, 65536 - 1] for n in (0, 1, 3, 258, 32767, 32768)]
    assert host(["run %d %d" % c for c in cases]) == [pieces(*c) for c in cases]
    ns = [0, 1, 32767, 32768, 32769, 65535]
    assert host(["skip %d" % n for n in ns]) == [[max(n - W, 0)] for n in ns]


def test_the_source_of_a_match(host):
    assert host(["mods"]) == [[1]]
    rnd = random.Random(1)
    cases = [(65536 + 5, d, n, i) for n in (3, 4, 17, 258) for d in (1, 2, n - 1, n, 16, 32767, 32768) for i in {0, 1, n // 2, n - 1}]
    cases += [(rnd.randrange(32768, 1 << 32), d, n, rnd.randrange(n)) for d, n in ((rnd.randrange(1, 300), rnd.randrange(3, 259)) for _ in range(200))]
    assert host(["src %d %d %d %d" % c for c in cases]) == [[at - d + (i % d if d < n else i)] for at, d, n, i in cases]


def test_a_ring_driven_through_the_rules_holds_the_last_window(host):
    """stored runs and matches with every distance of the hand-built streams, around several wraps, against a bytearray"""
    rnd = random.Random(2)
    out, ops, want = bytearray(), [], []
    for n, seed in ((65535, 3), (1, 9), (0, 0), (40000, 77)):
        ops.append("s %d %d %d" % (len(out), n, seed))
        out += bytes((seed + k) & 255 for k in range(n))
    while len(out) < 6 * W:
        gap = -len(out) % W
        n = 258 if 1 <= gap <= 257 else rnd.choice(B.LENS)
        d = rnd.choice((1, 2, n - 1, n, 16, W - 1, W))
        u = len(out)
        ops.append("m %d %d %d" % (u, d, n))
        for i in range(n):
            out.append(out[u - d + i])
        if rnd.random() < 0.05 or 1 <= gap <= 257:
            ops.append("d %d" % len(out))
            win = out[-W:]
            want += [sum(b * (k + 1) for k, b in enumerate(win)), len(win)]
    assert len(want) >= 20
    assert host(["ring " + " ".join(ops)]) == [want]


def test_the_hand_built_streams(host):
    """what the issue asks of them is asserted in checkpoint_build_cases.streams(); here: the model walks them to the same length"""
    s = B.streams()
    assert [x[0] for x in s] == ["far_fixed", "far_stored"]
    for name, fmt, stream, plain in s:
        for span in (258, 4096):
            m = F.index(stream, fmt, span)
            assert m is not None and m["out_len"] == len(plain) and m["count"] >= len(plain) // span, name
