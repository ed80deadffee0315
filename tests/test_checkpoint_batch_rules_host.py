"""The rules of the batched range read (power-gzip_amd/csrc/nxz_checkpoint_batch.h) -- the code the kernels of
nxz_checkpoint_batch.hip run wherever they decide what may be read -- compiled for the host under AddressSanitizer and UBSan
(tests/native/checkpoint_batch_host.cpp) and held against Python integers: a row's verdict, the bases, the flat uoff, the range
mapping, the row-to-slot mapping and the sums at the edge of 64 bits.  Every array reaches the rules as a heap block of exactly its
size: a stale row that made them read behind its own part would stop the program."""
import os
import random
import subprocess

import pytest

import checkpoint_fine_model as F
import checkpoint_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, OOB, BAD_STREAM = 0, 1, 4
CPS_OK, CPS_STREAM_FAILED, CPS_MORE, CPS_NO_OUTPUT, CPS_INVALID = range(5)
M64 = (1 << 64) - 1


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    exe = tmp_path_factory.mktemp("cpb") / "checkpoint_batch_host"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "power-gzip_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "checkpoint_batch_host.cpp"), "-o", str(exe)], check=True)

    def run(lines):
        r = subprocess.run([str(exe)], input=("\n".join(lines) + "\n").encode(), capture_output=True, timeout=600)
        assert r.returncode == 0, (r.returncode, r.stderr.decode()[-4000:])
        out = r.stdout.decode().splitlines()
        assert len(out) == len(lines)
        return [[int(x) for x in line.split()] for line in out]
    return run


# ---- the rules once more, in Python integers ---------------------------------------------------------------------------------------
def entry_ok(cbit, uoff, L, j, src_len):
    """rule 5 of include/nxz_engine.h for entry j of L checkpoints"""
    c0, c1, u0, u1 = cbit[j], cbit[j + 1], uoff[j], uoff[j + 1]
    if src_len > M64 >> 3 or c1 > 8 * src_len or c1 <= c0 or (j == 0 and u0 != 0):
        return False
    if (u1 <= u0) if j + 1 < L else (u1 < u0):
        return False
    return min(u0, 32768) + ((c1 + 7) >> 3) - (c0 >> 3) <= 0xffffffff and u1 - u0 <= 0xffffffff


def state_ok(s, j, cbit_j):
    """the per-entry checks listed at nxz_checkpoint_read_ranges_fine"""
    tbit, resume, dhtlen = s
    sfbt, rem = (resume >> 16) & 15, resume & 0xffff
    if resume >> 20 or (j == 0 and resume) or (sfbt and not 8 <= sfbt <= 0xd):
        return False
    if (rem == 0 or cbit_j & 7) if sfbt & 0xe == 8 else rem != 0:
        return False
    if sfbt & 0xe == 0xc:
        return 1 <= dhtlen <= 8 * 288 and tbit >= 3 and tbit + dhtlen <= cbit_j
    return tbit == 0 and dhtlen == 0


def row_ok(status, count, cp_cap, have_src, src_len, cbit, uoff, state=None):
    if status != CPS_OK or not 1 <= count <= cp_cap or not have_src:
        return False
    return all(entry_ok(cbit, uoff, count, k, src_len) and (state is None or state_ok(state[k], k, cbit[k])) for k in range(count))


def row_line(status, count, cp_cap, have_src, src_len, cbit, uoff, state=None):
    n = len(cbit)
    assert len(uoff) == n and (state is None or len(state) == n)
    tail = " " + " ".join("%d %d %d" % s for s in state) if state is not None else ""
    return "row %d %d %d %d %d %d %d %s %s%s" % (status, count, cp_cap, have_src, src_len, state is not None, n, " ".join(map(str, cbit)),
                                                 " ".join(map(str, uoff)), tail)


@pytest.fixture(scope="module")
def indexes():
    """a coarse index of five checkpoints and a fine one with stored, fixed and dynamic states"""
    s = {x[0]: x for x in F.streams()}
    text_stream = s["mem1"][2]                                           # (small blocks: a header every few KiB)
    co = M.index(text_stream, s["mem1"][1], 16384)
    assert 5 <= co["count"] <= 8
    fine = {name: (F.index(s[name][2], s[name][1], 4096), len(s[name][2])) for name in ("alice6_gzip_fields", "stored", "fixed_one_block")}
    return (co, len(text_stream)), fine


# ---- a row's verdict ---------------------------------------------------------------------------------------------------------------
def test_the_verdict_of_a_coarse_row(host, indexes):
    (co, src_len), _ = indexes
    n, cb, uo = co["count"], co["cbit"], co["uoff"]
    cases = [("the index", CPS_OK, n, n, 1, src_len, cb, uo), ("room to spare", CPS_OK, n, n + 7, 1, src_len, cb, uo),
             ("count 0", CPS_OK, 0, n, 1, src_len, [], []), ("count 0, entries there", CPS_OK, 0, n, 1, src_len, cb, uo),
             ("count > cp_cap", CPS_OK, n, n - 1, 1, src_len, [], []), ("count far beyond", CPS_OK, 0xffffffff, n, 1, src_len, [], []),
             ("no source", CPS_OK, n, n, 0, src_len, [], []), ("the source shorter", CPS_OK, n, n, 1, (cb[n] + 7) // 8 - 1, cb, uo),
             ("the source just long enough", CPS_OK, n, n, 1, (cb[n] + 7) // 8, cb, uo)]
    cases += [("status %d" % st, st, n, n, 1, src_len, [], []) for st in (CPS_STREAM_FAILED, CPS_MORE, CPS_NO_OUTPUT, CPS_INVALID, 99)]
    mid = n // 2
    for what, k in (("first", 0), ("middle", mid), ("sentinel", n)):
        c2 = list(cb)
        c2[k] = cb[k + 1] if k < n else cb[n - 1]                          # cbit no longer increases at that entry
        cases.append(("cbit at the %s entry" % what, CPS_OK, n, n, 1, src_len, c2, uo))
        u2 = list(uo)
        u2[k] = (uo[k + 1] if k < n else uo[n - 1] - 1) if k else 1         # uoff[0] != 0; uoff repeats; the sentinel's falls
        cases.append(("uoff at the %s entry" % what, CPS_OK, n, n, 1, src_len, cb, u2))
    cases.append(("sentinel behind the source", CPS_OK, n, n, 1, src_len, cb[:n] + [8 * src_len + 1], uo))
    cases.append(("a segment of 2^32 bytes", CPS_OK, n, n, 1, src_len, cb, uo[:n] + [uo[n - 1] + (1 << 32)]))
    cases.append(("an empty final block", CPS_OK, n, n, 1, src_len, cb, uo[:n] + [uo[n - 1]]))
    cases.append(("a source too long for bits", CPS_OK, n, n, 1, (M64 >> 3) + 1, cb, uo))
    got = host([row_line(*c[1:]) for c in cases])
    want = [[int(row_ok(*c[1:]))] for c in cases]
    assert [c[0] for c, g, w in zip(cases, got, want) if g != w] == []
    good = {c[0] for c, w in zip(cases, want) if w == [1]}
    assert good == {"the index", "room to spare", "the source just long enough", "an empty final block"}


def test_the_verdict_of_a_fine_row(host, indexes):
    _, fine = indexes
    lines, want, what = [], [], []
    for name, (idx, src_len) in fine.items():
        n = idx["count"]
        args = (CPS_OK, n, n, 1, src_len, idx["cbit"], idx["uoff"])
        lines.append(row_line(*args, idx["state"])); want.append([1]); what.append((name, "the model's index"))
        lines.append(row_line(*args)); want.append([1]); what.append((name, "without the states"))
        for w, b in F.broken_states(idx):
            a = (CPS_OK, n, n, 1, src_len, b["cbit"], b["uoff"])
            assert not row_ok(*a, b["state"]), (name, w)
            lines.append(row_line(*a, b["state"])); want.append([0]); what.append((name, w))
    got = host(lines)
    assert [w for g, x, w in zip(got, want, what) if g != x] == []
    assert len({w for _, w in what}) >= 19                               # every per-entry check of the fine reader, by name


# ---- the layout --------------------------------------------------------------------------------------------------------------------
def test_the_shape_the_call_takes(host):
    cases = [(1, 1), (0, 5), (5, 0), ((1 << 31) - 1, 1), (1 << 31, 1), (1 << 16, (1 << 16) - 1), (65535, 65536), (4096, 16), (1, 0xffffffff), (2, 0xffffffff),
             (1 << 40, 1)]
    want = [[int(c != 0 and n < 1 << 31 and n * (c + 1) < 1 << 32)] for n, c in cases]
    assert host(["shape %d %d" % c for c in cases]) == want
    assert want == [[1], [1], [0], [1], [0], [0], [1], [1], [0], [0], [0]]


def test_row_to_slot_at_the_far_corner(host):
    cases = [(0, 0, 8), (5, 7, 8), (5, 8, 8), (4095, 15, 16), (65534, 65535, 65536), ((1 << 31) - 2, 0, 1), (0, 0xfffffffe, 0xfffffffe)]
    for row, k, cap in cases:                                            # row = n_jobs - 1, k = cp_cap - 1 of the largest batches
        assert (row + 1) * (cap + 1) < 1 << 32
    want = [[row * (cap + 1) + k, row, k, row * cap + k, (row * cap + k) * 32768] for row, k, cap in cases]
    assert host(["slot %d %d %d" % c for c in cases]) == want
    assert all(w[4] + 32768 <= (1 << 32) * 32768 for w in want)


# ---- bases, the flat uoff and the ranges -------------------------------------------------------------------------------------------
def batch_model(rows, cp_cap, ranges, with_state):
    """rows: [(status, count, have_src, src_len, cbit[cp_cap + 1], uoff[cp_cap + 1], state[cp_cap + 1])] -> what the host program prints"""
    bad = [0 if row_ok(st, cnt, cp_cap, hs, sl, cb, uo, sta if with_state else None) else 1 for st, cnt, hs, sl, cb, uo, sta in rows]
    base = [0]
    for b, r in zip(bad, rows):
        base.append(base[-1] + (0 if b else r[5][r[1]]))
    fu, seg = [], []
    for i, (b, r) in enumerate(zip(bad, rows)):
        for k in range(cp_cap + 1):
            fu.append(base[i] if b else base[i] + r[5][k] if k <= r[1] else base[i + 1])
            seg.append(int(not b and k < r[1]))
    out = bad + base + fu + seg[:-1]
    for job, b, e in ranges:
        if job >= len(rows) or bad[job]:
            out += [BAD_STREAM, 0, 0]
        elif b > e or e > base[job + 1] - base[job]:
            out += [OOB, 0, 0]
        else:
            out += [OK, base[job] + b, base[job] + e]
    return out, bad, base, fu


def batch_line(rows, cp_cap, ranges, with_state):
    a = [len(rows), cp_cap, len(ranges), int(with_state)]
    for r in rows:
        a += list(r[:4])
    for f in (4, 5):
        for r in rows:
            a += r[f]
    if with_state:
        for r in rows:
            for s in r[6]:
                a += list(s)
    for q in ranges:
        a += list(q)
    return "batch " + " ".join(map(str, a))


def padded(idx, cp_cap, junk):
    """a row of cp_cap + 1 entries as an index call leaves it: the entries behind the sentinel are whatever was there"""
    n = idx["count"] + 1
    st = idx.get("state") or [(0, 0, 0)] * n
    return (idx["cbit"] + [junk] * (cp_cap + 1 - n), idx["uoff"] + [junk] * (cp_cap + 1 - n), st + [(junk, junk & 0xffffffff, 7)] * (cp_cap + 1 - n))


def test_bases_flat_uoff_and_ranges_of_a_mixed_batch(host, indexes):
    (co, co_len), fine = indexes
    fx, fx_len = fine["fixed_one_block"]
    cp_cap = max(co["count"], 8)
    short = {"cbit": [16, 200], "uoff": [0, 21], "count": 1}
    empty = {"cbit": [16, 26], "uoff": [0, 0], "count": 1}
    stale = dict(co, cbit=co["cbit"][:2] + [co["cbit"][1]] + co["cbit"][3:])
    junk = M64 - 3
    rows = [(CPS_OK, co["count"], 1, co_len) + padded(co, cp_cap, junk), (CPS_OK, 1, 1, 30) + padded(short, cp_cap, junk),
            (CPS_STREAM_FAILED, 0, 1, 500) + ([junk] * (cp_cap + 1), [junk] * (cp_cap + 1), [(junk, 5, 5)] * (cp_cap + 1)),
            (CPS_OK, 1, 1, 30) + padded(empty, cp_cap, 0), (CPS_MORE, cp_cap + 3, 1, co_len) + padded(co, cp_cap, junk),
            (CPS_OK, co["count"], 1, co_len) + padded(stale, cp_cap, junk), (CPS_OK, co["count"], 1, co_len) + padded(co, cp_cap, 1)]
    n_out = co["out_len"]
    ranges = [(0, 0, n_out), (0, 5, 5), (0, n_out, n_out), (0, 0, n_out + 1), (0, 9, 8), (1, 0, 21), (1, 20, 22), (2, 0, 1), (2, 0, 0), (3, 0, 0), (3, 0, 1),
              (4, 0, 1), (5, 0, 1), (6, 100, 70000), (7, 0, 0), (0xffffffff, 0, 0), (6, M64, M64), (6, 0, M64), (6, M64, 0)]
    for with_state in (False, True):
        want, bad, base, fu = batch_model(rows, cp_cap, ranges, with_state)
        assert host([batch_line(rows, cp_cap, ranges, with_state)]) == [want]
        assert bad == [0, 0, 1, 0, 1, 1, 0] and base[-1] == 2 * n_out + 21
        assert all(a <= b for a, b in zip(fu, fu[1:])) and fu[-1] == base[-1]          # the flat uoff never decreases: the map's search holds
    # ... and a fine row among coarse ones, with the states looked at
    rows = [rows[0], (CPS_OK, fx["count"], 1, fx_len) + padded(fx, fx["count"] + 2, junk)]
    rows[0] = (CPS_OK, co["count"], 1, co_len) + padded(co, fx["count"] + 2, junk)
    want, bad, base, fu = batch_model(rows, fx["count"] + 2, [(1, 0, fx["out_len"]), (1, 1, fx["out_len"] + 1)], True)
    assert host([batch_line(rows, fx["count"] + 2, [(1, 0, fx["out_len"]), (1, 1, fx["out_len"] + 1)], True)]) == [want] and bad == [0, 0]


def test_random_batches(host):
    rng = random.Random(11)
    lines, wants = [], []
    for _ in range(60):
        cp_cap, rows = rng.randrange(1, 6), []
        for _ in range(rng.randrange(1, 7)):
            count = rng.randrange(0, cp_cap + 2)
            cb, uo = [rng.randrange(0, 64)], [0 if rng.random() < 0.9 else 1]
            for k in range(cp_cap):
                cb.append(cb[-1] + rng.choice([1, 9, 200, 0]) if rng.random() < 0.95 else 0)
                uo.append(uo[-1] + rng.choice([1, 40000, 1 << 31, 0]) if rng.random() < 0.95 else 3)
            rows.append((rng.choice([CPS_OK] * 5 + [CPS_MORE, CPS_STREAM_FAILED]), count, int(rng.random() < 0.95), rng.choice([(max(cb) + 7) // 8, 10]), cb, uo,
                         [(0, 0, 0)] * (cp_cap + 1)))
        ranges = []
        for _ in range(12):
            b = rng.choice([0, 1, 40000, 1 << 31, rng.randrange(1 << 33)])
            ranges.append((rng.randrange(len(rows) + 1), b, rng.choice([b, b + 1, b + 40000, max(b - 1, 0), rng.randrange(1 << 33)])))
        lines.append(batch_line(rows, cp_cap, ranges, False))
        wants.append(batch_model(rows, cp_cap, ranges, False)[0])
    got = host(lines)
    assert [i for i, (g, w) in enumerate(zip(got, wants)) if g != w] == []
    stats = [w[-3 * 12::3] for w in wants]
    assert {OK, OOB, BAD_STREAM} <= {s for st in stats for s in st}


def test_sums_at_the_edge_of_64_bits(host):
    """every extent is at most count * (2^32 - 1) (rule 5), and the shape bounds the counts of a batch: the largest batches the call
    takes cannot carry a base beyond 2^64 - 1, so the kernels add without a check"""
    top = host(["extmax %d" % c for c in (0, 1, 0xffffffff)])
    assert top == [[0], [0xffffffff], [0xffffffff * 0xffffffff]]
    for n_jobs, cp_cap in ((65535, 65536), ((1 << 31) - 1, 1), (1, 0xfffffffe), (4096, 16)):
        assert host(["shape %d %d" % (n_jobs, cp_cap)]) == [[1]]
        assert n_jobs * cp_cap * 0xffffffff <= M64
    # bases as close to the edge as that allows, and beyond what it allows: the mapping itself never wraps inside a row's extent
    base = [0, M64 - 10, M64 - 10, M64]
    cases = [(2, 0, 10), (2, 10, 10), (2, 0, 11), (2, 11, 11), (0, M64 - 10, M64 - 10), (0, 0, M64 - 9), (1, 0, 0), (1, 0, 1), (2, M64, M64), (3, 0, 0)]
    want = []
    for job, b, e in cases:
        ext = base[job + 1] - base[job] if job < 3 else None
        want.append([BAD_STREAM, 0, 0] if ext is None else [OOB, 0, 0] if b > e or e > ext else [OK, base[job] + b, base[job] + e])
    assert host(["map %d %d %d 3 0 0 0 %s" % (c + (" ".join(map(str, base)),)) for c in cases]) == want
    assert want[0] == [OK, M64 - 10, M64] and want[2] == [OOB, 0, 0]
    assert host(["map 1 0 0 3 0 1 0 %s" % " ".join(map(str, base))]) == [[BAD_STREAM, 0, 0]]
