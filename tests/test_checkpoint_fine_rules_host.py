"""The rules of the fine checkpoint calls (power-gzip_amd/csrc/nxz_checkpoint_fine.h) -- the code the kernels of
nxz_checkpoint_fine.hip run -- compiled for the host under AddressSanitizer and UBSan (tests/native/checkpoint_fine_host.cpp) and held
against the Python model (tests/checkpoint_fine_model.py): the budget rule on token lists, the state entry, the validity of an index
with its states, the job fields of a segment and the bytes of its table slot."""
import os
import random
import subprocess

import pytest

import checkpoint_fine_model as F
import checkpoint_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DHT_SLOT = 288 + 4


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    exe = tmp_path_factory.mktemp("cpf") / "checkpoint_fine_host"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "power-gzip_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "checkpoint_fine_host.cpp"), "-o", str(exe)], check=True)

    def run(lines):
        r = subprocess.run([str(exe)], input=("\n".join(lines) + "\n").encode(), capture_output=True, timeout=600)
        assert r.returncode == 0, (r.returncode, r.stderr.decode()[-4000:])
        out = r.stdout.decode().splitlines()
        assert len(out) == len(lines)
        return [[int(x) for x in line.split()] for line in out]
    return run


def test_the_header_has_the_struct_and_the_constants():
    hdr = open(os.path.join(ROOT, "include", "nxz_engine.h")).read()
    assert "typedef struct nxz_checkpoint_state {" in hdr and "#define NXZ_DHT_MAXSZ  288" in hdr and "#define NXZ_JOB_SUSPEND_WHEN_FULL 1u" in hdr
    rules = open(os.path.join(ROOT, "power-gzip_amd", "csrc", "nxz_checkpoint_fine.h")).read()
    assert "#define NXZ_CPF_SPAN_MIN 258u" in rules and F.SPAN_MIN == 258 and F.DHT_MAXSZ == 288


def test_span_and_budget(host):
    assert host(["span 0", "span 257", "span 258", "span %d" % (1 << 40)]) == [[0], [0], [1], [1]]
    cases = [(0, 258, 0xffffffff), (1000, 4096, 0xffffffff), (0xfffffff0, 4096, 0xffffffff), (5, 1 << 63, 0xffffffff), (5, (1 << 64) - 1, 0xffffffff),
             (100, 300, 350), (100, 300, 400), (100, 300, 401)]
    assert host(["budget %d %d %d" % c for c in cases]) == [[min(c[0] + c[1], c[2])] for c in cases]


def model_rule(span, cp_cap, toks):
    """toks: [(n, count)] -> [count, k_1, u_1, ...] by the rule of checkpoint_fine_model.index"""
    u, c, count, stored = 0, 0, 1, []
    for n, cnt in toks:
        for _ in range(cnt):
            if u + n > c + span:
                if count < cp_cap:
                    stored += [count, u]
                count += 1
                c = u
            u += n
    return [count] + stored


def test_budget_rule_on_token_lists(host):
    rng = random.Random(7)
    cases = [(258, 8, [(258, 5)]), (258, 8, [(1, 258), (1, 1)]), (258, 8, [(1, 257), (258, 1)]), (1000, 64, [(1, 1), (258, 40)]),
             (4096, 4, [(1, 65535), (1, 65535)]),                          # stored runs, counted past cp_cap
             (1 << 33, 4, [(258, 1000)])]                                  # a span beyond 32 bits: no checkpoint
    for _ in range(100):
        span = rng.choice([258, 259, 300, 1000, 4096])
        toks = [(rng.choice([1, 1, 3, 17, 258, rng.randrange(3, 259)]), rng.randrange(1, 400 if rng.random() < 0.2 else 8)) for _ in range(rng.randrange(1, 60))]
        cases.append((span, rng.choice([1, 3, 1000]), toks))
    got = host(["rule %d %d %d %s" % (s, cap, len(t), " ".join("%d %d" % x for x in t)) for s, cap, t in cases])
    for (s, cap, t), g in zip(cases, got):
        assert g == model_rule(s, cap, t), (s, cap, t)
    assert got[0] == [5, 1, 258, 2, 516, 3, 774, 4, 1032] and got[1] == [2, 1, 258] and got[2] == [2, 1, 257]
    assert got[3][0] == 1 + (1 + 258 * 40 - 1) // 774 and got[3][1:5] == [1, 775, 2, 1549]        # 1 + 3 x 258, then 3 x 258 each
    assert got[4] == [1 + (2 * 65535 - 1) // 4096, 1, 4096, 2, 8192, 3, 12288] and got[5] == [1]


def test_the_rule_on_real_token_lists(host):
    for name, fmt, stream, plain in F.streams():
        if plain is None or name not in ("fixed_one_block", "stored", "mem1", "rle_zeros"):
            continue
        tokens = F.walk_cached(stream, fmt)[0]
        for span in (258, 1000, 65536):
            idx = F.index(stream, fmt, span)
            g = host(["rule %d %d %d %s" % (span, 1 << 20, len(tokens), " ".join("%d %d" % (t[2], t[3]) for t in tokens))])[0]
            assert g[0] == idx["count"] and g[2::2] == idx["uoff"][1:idx["count"]], (name, span)


def test_state_entries(host):
    cases = [(0, 0, 0, 0), (0, 7, 99, 99), (0x8, 65535, 5, 5), (0x9, 1, 0, 0), (0xa, 9, 7, 7), (0xb, 0, 0, 0), (0xc, 3, 19, 500), (0xd, 0, 1 << 40, 2304)]
    want = [list(F.state_entry(s, r, t, d)) if s else [0, 0, 0] for s, r, t, d in cases]
    want = [[w[0], w[1] if (c[0] & 0xe) == 8 else c[0] << 16, w[2]] for w, c in zip(want, cases)]
    assert host(["state %d %d %d %d" % c for c in cases]) == want
    assert want[2] == [0, 65535 | 8 << 16, 0] and want[4] == [0, 0xa << 16, 0] and want[6] == [19, 0xc << 16, 500]


def valid_line(src_len, idx):
    n = len(idx["cbit"])
    return "valid %d %d %s %s %s" % (src_len, n, " ".join(map(str, idx["cbit"])), " ".join(map(str, idx["uoff"])),
                                     " ".join("%d %d %d" % s for s in idx["state"]))


def test_validity(host):
    lines, want, what = [], [], []
    for name, fmt, stream, plain in F.streams():
        if plain is None or name not in ("alice6_gzip_fields", "stored", "fixed_one_block", "mem1"):
            continue
        idx = F.index(stream, fmt, 1000)
        lines.append(valid_line(len(stream), idx)); want.append([1]); what.append((name, "the model's index"))
        for w, b in F.broken_states(idx):
            lines.append(valid_line(len(stream), b)); want.append([0]); what.append((name, w))
        # a coarse index with a zeroed state array
        co = M.index(stream, fmt, 16384)
        co["state"] = [(0, 0, 0)] * len(co["cbit"])
        lines.append(valid_line(len(stream), co)); want.append([1]); what.append((name, "coarse, zero states"))
        # ... and what the coarse rules refuse stays refused
        bad = dict(idx, cbit=idx["cbit"][:-1] + [8 * len(stream) + 1])
        lines.append(valid_line(len(stream), bad)); want.append([0]); what.append((name, "sentinel behind the source"))
    got = host(lines)
    assert [w for g, x, w in zip(got, want, what) if g != x] == []
    assert len({w for _, w in what}) >= 19


def test_segment_job_fields_and_table_slot(host):
    name, fmt, stream, plain = next(s for s in F.streams() if s[0] == "alice6_gzip_fields")
    idx = F.index(stream, fmt, 4096)
    ks = [k for k in range(idx["count"]) if idx["state"][k][2]][:12] + [0]
    jobs = host(["job %d %d %d %d" % (idx["state"][k] + (idx["cbit"][k],)) for k in ks])
    for k, j in zip(ks, jobs):
        assert j == [idx["state"][k][1] | ((8 - (idx["cbit"][k] & 7)) & 7) << 20, 1], k
    # the slot from a source cut right behind the table's last bit: no byte behind it is read (AddressSanitizer watches)
    lines, want = [], []
    for k in ks[:-1]:
        tbit, _, dhtlen = idx["state"][k]
        cut = stream[:(tbit + dhtlen + 7) // 8]
        lines.append("dht %d %d %d %s" % (tbit, dhtlen, len(cut), " ".join(map(str, cut))))
        want.append(list(F.table_bits(stream, tbit, dhtlen).ljust(DHT_SLOT, b"\0")))
    rng = random.Random(3)
    for _ in range(40):                                                  # any alignment, any length, ones all around
        tbit, dhtlen = rng.randrange(3, 64), rng.randrange(1, 8 * 288 + 1)
        src = bytes([0xff]) * ((tbit + dhtlen + 7) // 8)
        lines.append("dht %d %d %d %s" % (tbit, dhtlen, len(src), " ".join(map(str, src))))
        want.append(list(F.table_bits(src, tbit, dhtlen).ljust(DHT_SLOT, b"\0")))
    assert host(lines) == want
