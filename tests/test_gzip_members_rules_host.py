"""The rules of the multi-member gzip calls (power-gzip_amd/csrc/nxz_gzip_members.h) -- the code the kernels of
nxz_gzip_members.hip run -- compiled for the host under AddressSanitizer and UBSan (tests/native/gzip_members_host.cpp) and held
against the Python model (tests/gzip_members_model.py): the continue / stop / fail decisions, the uoff / consumed arithmetic, the
member cap, and the decode's plan and join.  The harness gets, per member, what a header parser and a deflate walk found (here:
tests/framing.py and zlib); everything decided from there on is the header's."""
import os
import random
import subprocess
import zlib

import pytest

import framing as F
import gzip_members_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    exe = tmp_path_factory.mktemp("gzm") / "gzip_members_host"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "power-gzip_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "gzip_members_host.cpp"), "-o", str(exe)], check=True)

    def run(lines):
        r = subprocess.run([str(exe)], input=("\n".join(lines) + "\n").encode(), capture_output=True, timeout=600)
        assert r.returncode == 0, (r.returncode, r.stderr.decode()[-4000:])
        return r.stdout.decode().splitlines()
    return run


def facts(src, pos):
    """what the kernel's parser and walk find at src[pos:]: header status and length, the walk's cc / final_eob, deflate bytes used, bytes counted"""
    left = src[pos:]
    f = F.parse(left, F.FMT_GZIP)
    if f["status"] != F.OK:
        return (f["status"], 0, 0, 0, 0, 0)
    hl = f["hdr_len"]
    body = left[hl:max(hl, len(left) - 8)]
    d = zlib.decompressobj(-15)
    try:
        out = d.decompress(body)
    except zlib.error:
        return (F.OK, hl, 66, 0, 0, 0)
    if not d.eof:
        return (F.OK, hl, 0, 0, len(body), len(out))
    return (F.OK, hl, 0, 1, len(body) - len(d.unused_data), len(out))


def ask(host, src, cap):
    """the header's walk over src, fed the facts at every member start the MODEL visits (and one beyond, should the rules go on)"""
    s, recs, _ = M.walk(src)
    starts = [m["coff"] for m in recs] + [s["consumed"]]
    lines = ["walk %d %d %s %d" % (cap, len(src), src.hex() or "-", len(starts))] + ["%d %d %d %d %d %d" % facts(src, p) for p in starts]
    out = host(lines)
    got_s = [int(x) for x in out[-1].split()[1:]]
    got_m = [[int(x) for x in line.split()] for line in out[:-1]]
    return got_s, got_m


def hold(host, src, cap):
    s, recs, _ = M.walk(src, cap)
    got_s, got_m = ask(host, src, cap)
    assert got_s[:5] == [s[k] for k in M.STREAM_FIELDS], (cap, got_s, s)
    assert got_m == [[m[k] for k in M.MEMBER_FIELDS] for m in recs], cap
    return s, got_s


def jobs():
    rnd = random.Random(12)
    ms = [M.mixed_member(rnd, k) for k in range(17)]
    cat = b"".join
    flip = lambda b, i, m=1: b[:i] + bytes([b[i] ^ m]) + b[i + 1:]
    big = M.gz(M.payload(rnd, 2000), 6, **M.HEADERS[5])       # a header of 220 bytes, every optional field
    h3 = F.parse(ms[3], F.FMT_GZIP)["hdr_len"]
    out = {
        "one": ms[1], "two": cat(ms[:2]), "three": cat(ms[:3]), "seventeen": cat(ms), "empties": M.gz(b"") * 3,
        "zeros": cat(ms[:3]) + bytes(7), "one_zero": cat(ms[:3]) + b"\0", "garbage": cat(ms[:3]) + b"\x1f\x8cgarbage", "half_magic": cat(ms[:3]) + b"\x1f",
        "bad_method": cat(ms[:3]) + b"\x1f\x8b\x07\x00", "magic_only": cat(ms[:2]) + b"\x1f\x8b", "bad_flags": cat(ms[:2]) + b"\x1f\x8b\x08\xe0" + bytes(20),
        "cut_header": ms[1] + big[:5], "cut_name": ms[1] + big[:100], "cut_deflate": ms[1] + big[:len(big) // 2],
        "cut_trailer": ms[1] + big[:-3], "cut_all_trailer": ms[1] + big[:-8], "first_cut": ms[1][:40],
        "bad_isize": ms[1] + flip(ms[2], len(ms[2]) - 2) + ms[3], "bad_crc": ms[1] + flip(ms[2], len(ms[2]) - 6) + ms[3],
        "bad_hcrc": ms[1] + flip(ms[4], 3, 1) + ms[3], "bad_deflate": ms[1] + ms[3][:h3] + bytes([ms[3][h3] | 6]) + ms[3][h3 + 1:],
        "nothing": b"", "not_gzip": b"plain text",
    }
    return out


def test_walk_decisions_and_sums(host):
    seen = set()
    for name, src in jobs().items():
        for cap in (1, 2, 3, 16, 17, 18):
            s, got = hold(host, src, cap)
            seen.add(s["status"])
    assert seen == {M.GZS_OK, M.GZS_MEMBER_FAILED, M.GZS_MORE_MEMBERS}


def test_named_outcomes(host):
    """the cases of the rules, spelled out (not only "equal to the model")"""
    j = jobs()
    three = len(j["three"])
    for name in ("zeros", "one_zero", "garbage", "half_magic"):
        s, _ = hold(host, j[name], 8)
        assert (s["status"], s["members"], s["failed"], s["consumed"]) == (M.GZS_OK, 3, 3, three), name
    s, got = hold(host, j["bad_method"], 8)
    assert (s["status"], s["members"], s["failed"], s["consumed"]) == (M.GZS_MEMBER_FAILED, 4, 3, three)
    assert ask(host, j["bad_method"], 8)[1][3][6] == F.BAD_METHOD
    for name in ("cut_header", "cut_name", "cut_deflate", "cut_trailer", "cut_all_trailer"):
        s, got = hold(host, j[name], 8)
        assert (s["status"], s["members"], s["failed"]) == (M.GZS_MEMBER_FAILED, 2, 1), name
        assert ask(host, j[name], 8)[1][1][6] == F.TRUNCATED, name
    assert got[5] == 3                                      # cc of a member whose deflate data was cut short
    assert ask(host, j["bad_isize"], 8)[1][1][6] == F.BAD_LENGTH
    s, _ = hold(host, j["bad_crc"], 8)
    assert (s["status"], s["members"]) == (M.GZS_OK, 3)     # the size pass cannot see a wrong CRC
    assert ask(host, j["bad_hcrc"], 8)[1][1][6] == F.BAD_HCRC
    s, got = hold(host, j["bad_deflate"], 8)
    assert ask(host, j["bad_deflate"], 8)[1][1][6] == F.DEFLATE and got[5] == 66
    s, _ = hold(host, j["seventeen"], 2)
    assert (s["status"], s["members"], s["failed"]) == (M.GZS_MORE_MEMBERS, 17, 17) and s["out_len"] == len(M.plain(j["seventeen"])[0])
    s, _ = hold(host, j["nothing"], 4)
    assert (s["status"], s["members"], s["failed"]) == (M.GZS_MEMBER_FAILED, 1, 0)
    assert host(["refused"])[0].split()[1:] == ["4", "0", "0", "0", "0", "0"]
    assert host(["job 0 0", "job 1 0", "job 0 1", "job %d 0" % 0x00e80000]) == ["1", "0", "0", "0"]


def test_random_series(host):
    rnd = random.Random(5)
    for _ in range(40):
        ms = [M.mixed_member(rnd, rnd.randrange(100), rnd.randrange(0, 400)) for _ in range(rnd.randrange(1, 9))]
        src = b"".join(ms) + rnd.choice([b"", b"\0\0\0", b"\x1f", b"\x1f\x8b", b"tail"])
        if rnd.randrange(3) == 0:
            src = src[:rnd.randrange(len(src) + 1)]
        hold(host, src, rnd.choice([1, 2, 4, 8]))
        out, used = (b"", 0)
        s, recs, outs = M.walk(src)
        if s["status"] == M.GZS_OK:                         # and the model against zlib's own loop over the members
            out, used = M.plain(src)
            assert (s["out_len"], s["consumed"]) == (len(out), used) and b"".join(outs) == out


def test_sums_past_4_gib(host):
    """uoff and out_len are 64-bit sums: members of nearly 2^32 bytes each, as the walk would report them"""
    m = M.gz(b"x")
    big = 0xfffffff0
    tr = (big).to_bytes(4, "little")
    fake = m[:-4] + tr
    src = fake * 3
    f = facts(m, 0)
    line = "%d %d %d %d %d %d" % (f[0], f[1], f[2], f[3], f[4], big)
    out = host(["walk 8 %d %s 3" % (len(src), src.hex()), line, line, line])
    assert [int(x.split()[0]) for x in out[:3]] == [0, big, 2 * big]
    assert out[3].split()[1:6] == ["0", "3", "3", str(len(src)), str(3 * big)]


def test_records_inside_their_job(host):
    q = lambda st, coff, clen, uoff, isize, sl, dc: "inside %d %d %d %d %d %d %d" % (st, coff, clen, uoff, isize, sl, dc)
    lines = [q(0, 0, 100, 0, 50, 100, 50), q(0, 1, 100, 0, 50, 100, 50), q(0, 0, 100, 1, 50, 100, 50), q(0, 0, 100, 0, 51, 100, 50),
             q(7, 0, 100, 0, 50, 100, 50), q(0, 0xffffffff, 0xffffffff, 0, 0, 0xffffffff, 0), q(0, 0, 0, 2 ** 40, 0, 10, 0xffffffff),
             q(0, 0, 0, 0xffffffff, 1, 10, 0xffffffff), q(0, 0, 0, 0xfffffffe, 1, 10, 0xffffffff), q(0, 100, 0, 50, 0, 100, 50)]
    assert host(lines) == ["1", "0", "0", "0", "0", "0", "0", "0", "1", "1"]


def test_plan_and_join(host):
    OK, FAILED, MORE, SPACE, INVALID = range(5)
    p = lambda *a: "plan %d %d %d %d %d %d %d %d" % a      # status out_len failed member_cap dst_cap stale base total
    cases = [(p(OK, 100, 3, 8, 100, 0, 0, 3), (OK, 3)), (p(OK, 100, 3, 8, 99, 0, 0, 3), (SPACE, 0)), (p(OK, 100, 3, 8, 100, 1, 0, 3), (INVALID, 0)),
             (p(MORE, 100, 9, 8, 100, 0, 0, 8), (MORE, 8)), (p(MORE, 100, 9, 8, 100, 0, 1, 8), (INVALID, 0)), (p(FAILED, 100, 2, 8, 100, 0, 5, 7), (FAILED, 2)),
             (p(FAILED, 0, 0, 8, 0, 0, 7, 7), (FAILED, 0)), (p(INVALID, 0, 0, 8, 100, 0, 0, 8), (INVALID, 0)), (p(SPACE, 10, 1, 8, 100, 0, 0, 8), (INVALID, 0)),
             (p(OK, 2 ** 32, 2, 8, 0xffffffff, 0, 0, 8), (SPACE, 0)), (p(FAILED, 100, 9, 4, 100, 0, 0, 4), (FAILED, 4))]
    out = host([c for c, _ in cases])
    assert [tuple(int(x) for x in line.split()) for line in out] == [w for _, w in cases]
    none = 0xffffffff
    out = host(["join %d 3 %d 0 100" % (OK, none), "join %d 3 1 0 60" % OK, "join %d 9 %d 0 100" % (MORE, none), "join %d 2 %d 0 100" % (FAILED, none),
                "join %d 2 0 67 40" % FAILED])
    assert out == ["0 3 100 0", "1 1 60 0", "2 9 100 0", "1 2 100 0", "1 0 40 67"]
