"""The rules of the batched verify (power-gzip_amd/csrc/nxz_verify.h) and the slice arithmetic they use (nxz_cksum_slices.h) -- the
code the kernel of nxz_inflate_verify.hip runs -- compiled for the host under AddressSanitizer and UBSan (tests/native/verify_host.cpp),
driven "as 64 lanes would" over a 32 KiB ring and held against zlib.crc32 / zlib.adler32 of the same prefix after every pass and at
the end; and the geometry alone: a pass never runs ahead of the output and never reaches back further than the ring holds."""
import os
import random
import subprocess
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W = 32768
NOCAP = 0xffffffff


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    exe = tmp_path_factory.mktemp("verify") / "verify_host"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "power-gzip_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "verify_host.cpp"), "-o", str(exe)], check=True)

    def run(lines):
        r = subprocess.run([str(exe)], input=("\n".join(lines) + "\n").encode(), capture_output=True, timeout=600)
        assert r.returncode == 0, (r.returncode, r.stderr.decode()[-4000:])
        out = r.stdout.decode().splitlines()
        assert len(out) == len(lines)
        return [[int(x) for x in line.split()] for line in out]
    return run


@pytest.fixture(scope="module")
def C(host):
    pass_, lanes, ring = host(["consts"])[0]
    assert lanes == 64 and ring == W
    assert pass_ % 64 == 0 and 258 <= pass_ <= W - 64          # a token always fits a fresh budget; a pass's bytes are still in the ring
    return pass_


def gen(seed, n):
    """verify_host.cpp's generator: output byte k of a drive with this seed"""
    k = np.arange(n, dtype=np.uint64)
    x = (np.uint64(seed) * np.uint64(2654435761) + k * np.uint64(40503)) & np.uint64(0xffffffff)
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(2246822519)) & np.uint64(0xffffffff)
    x ^= x >> np.uint64(13)
    return ((x >> np.uint64(8)) & np.uint64(0xff)).astype(np.uint8).tobytes()


def tokens(rng, n, stored_share=0.05):
    """token lengths 1..258 and now and then a stored run (up to 65535: longer than two passes) that add up to n"""
    toks, left = [], n
    while left:
        if rng.random() < stored_share:
            ln = min(left, rng.choice([1, 63, 64, 65, 5000, 40000, 65535]))
            toks.append("s%d" % ln)
        else:
            ln = min(left, rng.randint(1, 258))
            toks.append("t%d" % ln)
        left -= ln
    return toks


def check(host, C, n, toks, seed=1, in_crc=0, in_adler=1, win=0, cap=NOCAP, produced=None):
    out = host(["drive %d %d %d %d %d %d %s" % (n, seed, in_crc, in_adler, win, cap, " ".join(toks))])[0]
    plain = gen(seed, n)
    assert len(out) % 4 == 0 and out
    quads = [out[i:i + 4] for i in range(0, len(out), 4)]
    last_u = last_done = 0
    for u, done, crc, adler in quads[:-1]:
        assert last_done <= done <= u and done == u & ~63 and u - last_done <= W and last_u <= u <= last_u + C
        assert crc == zlib.crc32(plain[:done], in_crc) and adler == zlib.adler32(plain[:done], in_adler), (n, u, done)
        last_u, last_done = u, done
    u, done, crc, adler = quads[-1]
    assert u == done == (n if produced is None else produced) and u - last_done <= W
    assert crc == zlib.crc32(plain[:u], in_crc) and adler == zlib.adler32(plain[:u], in_adler), (n, u)
    return quads


def lengths(C):
    return [0, 1, 63, 64, 65, C - 1, C, C + 1, 32767, 32768, 32769, 65536 + 63, 200000]


def test_every_length_with_random_tokens_and_stored_runs(host, C):
    rng = random.Random(18)
    for n in lengths(C):
        quads = check(host, C, n, tokens(rng, n), seed=n + 1)
        assert len(quads) >= n // C            # (a cut a pass's worth of output at the latest, and the end)
    # nothing but one stored run, nothing but single bytes
    check(host, C, 65535, ["s65535"], seed=3)
    check(host, C, 3 * C + 7, ["t1"] * (3 * C + 7), seed=4)


def test_seeds_other_than_0_and_1(host, C):
    rng = random.Random(7)
    for n in (0, 1, 64, C + 1, 65536 + 63):
        check(host, C, n, tokens(rng, n), seed=n + 2, in_crc=0xdeadbeef, in_adler=0x12345678)
        check(host, C, n, tokens(rng, n), seed=n + 3, in_crc=0xffffffff, in_adler=(65520 << 16) | 65520)


def test_a_token_on_the_pass_edge_and_one_across_it(host, C):
    # the budget ends at C: a token that ends exactly there fits, the next one is cut in front of -- at C
    toks = ["t256"] * (C // 256) + ["t258", "t10"]
    quads = check(host, C, C + 268, toks, seed=5)
    assert [q[0] for q in quads] == [C, C + 268] and quads[0][1] == C
    # ... and one that would straddle it is cut in front of: at C - 1, where the pass leaves a slice unfinished
    toks = ["t255"] + ["t256"] * (C // 256 - 1) + ["t258", "t10"]
    quads = check(host, C, C + 267, toks, seed=6)
    assert [q[0] for q in quads] == [C - 1, C + 267] and quads[0][1] == C - 64
    # a stored run is split exactly at the edge
    quads = check(host, C, 2 * C + 5, ["t5", "s%d" % (2 * C)], seed=7)
    assert [q[0] for q in quads] == [C, 2 * C, 2 * C + 5]


def test_a_pass_whose_slices_end_at_the_ring_s_wrap(host, C):
    n = W + C
    quads = check(host, C, n, ["t256"] * (n // 256), seed=8)
    assert [q[1] for q in quads[:-1]] == list(range(C, n + 1, C))[:len(quads) - 1] and W in [q[1] for q in quads]
    # ... and passes that begin 63 bytes in front of a slice edge all the way round
    n = 3 * W
    check(host, C, n, ["t63"] + ["t256"] * ((n - 63) // 256) + ["t%d" % ((n - 63) % 256)], seed=9)


def test_a_preloaded_window_is_never_checksummed(host, C):
    rng = random.Random(3)
    for win in (1, 32767, 32768):
        for n in (0, 1, 100, C + 1, 32768, 65536 + 63):
            check(host, C, n, tokens(rng, n), seed=win + n, win=win)


def test_the_cap_ends_the_stream_where_the_walk_would(host, C):
    # below a pass's worth of the cap the budget is the cap itself: no cut is made, the token that does not fit ends the stream
    n = 3 * C
    toks = ["t258"] * (n // 258) + ["t%d" % (n % 258)]
    for cap in (0, 1, 258, C, C + 1, 2 * C + 100, n - 1, n):
        whole = min(cap // 258, n // 258) * 258
        produced = n if cap >= n else whole
        check(host, C, n, toks, seed=11, cap=cap, produced=produced)


def test_the_geometry_alone(host, C):
    rng = random.Random(1)
    caps = [0, 1, 63, 64, C - 1, C, C + 1, 2 * C, 1 << 31, NOCAP - 1, NOCAP]
    cuts = [0, 1, 63, 64, 65, C - 1, C, C + 1, W - 1, W, W + 1, (1 << 31) - 1, 1 << 31, NOCAP - C - 1, NOCAP - C, NOCAP - C + 1, NOCAP - 1, NOCAP]
    cuts += [rng.randrange(1 << 32) for _ in range(200)]
    cases = [(c, cap) for c in cuts for cap in caps + [c, min(c + C - 1, NOCAP), min(c + C, NOCAP), min(c + C + 1, NOCAP)] if c <= cap]
    got = host(["budget %d %d" % cc for cc in cases])
    req = []
    for (c, cap), (b,) in zip(cases, got):
        assert b == min(cap, c + C) and c <= b <= cap
        assert (b == cap) == (c + C >= cap)                     # cap itself once a pass's worth reaches it: the CC 13 path is the walk's
        done = c & ~63                                          # what the pass at the cut at c left
        for u in {c, b, (c + b) // 2, max(c, b - 1)}:
            assert u - done <= C + 63 <= W
            req.append((done, u))
    for (done, u), (ns,) in zip(req, host(["slices %d %d" % r for r in req])):
        assert 0 <= ns <= 256 and done + 64 * ns == u & ~63 and done + 64 * ns <= u and u - (done + 64 * ns) < 64
