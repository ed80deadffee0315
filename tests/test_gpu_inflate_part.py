"""GPU tests of nxz_batch_inflate_streams_part (include/nxz_engine.h; the kernels in power-gzip_amd/csrc/nxz_inflate_part.hip, the rules
in nxz_inflate_part.h): streams read in parts, a device buffer a part, the running state in a carry record on the device.  Every case
holds the device's bytes, per-part results and carry to tests/inflate_part_model.py (the CPU oracle part by part, proven against
zlib.decompressobj in tests/test_inflate_part_model_host.py); nothing is compared with the code under test.  The streams are
resume_cases.streams() (none above 70 000 plain bytes).

A scenario is one stream's calls.  The model runs first and says what every call must give -- in_used of a full target included,
so the call that sends the rest again is known up front -- and the device then gets ALL calls of all scenarios queued on one HIP
stream, a snapshot of the carry array behind each, and ONE wait at the end: the test reads nothing between the calls."""
import importlib
import os
import random
import struct
import zlib

import numpy as np
import pytest

import framing as F
import inflate_part_model as M
import resume_cases as R
from test_inflate_part_model_host import byte_parts, framed, many_part_splits, two_part_cuts

pytestmark = pytest.mark.gpu
pkg = importlib.import_module("power-gzip_amd")
E = pkg.engine
RAW, ZLIB, GZIP, AUTO = E.FMT_RAW, E.FMT_ZLIB, E.FMT_GZIP, E.FMT_AUTO
FIRST = E.PART_FIRST
CANARY = 0xc3
BIG = 1 << 20
STREAMS = R.streams()
BY_NAME = {s.name: s for s in STREAMS}


@pytest.fixture(scope="module")
def eng():
    e = pkg.Engine(0)
    yield e
    e.close()


class Step:
    """one call of a scenario: the part's bytes; flags (None: FIRST on the scenario's first call); the target's capacity; null: a
    pointer handed over as NULL ("src", "dst", "prev") with its length left as it is"""

    def __init__(self, src, flags=None, cap=BIG, null=None, prev_len=None):
        self.src, self.flags, self.cap, self.null, self.prev_len = src, flags, cap, null, prev_len


class Scenario:
    """fmt; steps; whole: the raw deflate data (where targets fill); prev: "contig" (the outputs lie end to end and prev is what lies
    in front of dst) or an int (prev is a copy elsewhere, at that byte offset from a 16-byte boundary); keep: the most output bytes
    handed over as prev; dst_align: where the first target lies from a 16-byte boundary; resend_caps: the targets of the calls that
    send the rest of a part again after a full target"""

    def __init__(self, fmt, steps, whole=None, prev="contig", keep=40000, dst_align=0, resend_caps=(BIG,), name=""):
        self.fmt, self.whole, self.prev, self.keep, self.dst_align, self.name = fmt, whole, prev, keep, dst_align, name
        self.calls = []                                                # (step, prev bytes, carry after, result, out)
        c, data, k = None, b"", 0
        queue = list(steps)
        while queue:
            st = queue.pop(0)
            flags = st.flags if st.flags is not None else (FIRST if not self.calls else 0)
            prev_b = b"" if flags & FIRST else data[data_at:][-keep:] if keep else b""
            if st.prev_len is not None:
                prev_b = data[len(data) - st.prev_len:] if st.prev_len else b""
            if st.null:
                cc = M.CC_INVALID_OP
                c2, r, out = c, dict(cc=cc, status=M.S_FAILED, in_used=0, out_len=0, crc=0, adler=0), b""
            else:
                c2, r, out = M.part(c, fmt, st.src, st.cap, prev_b, flags, whole)
            self.calls.append((Step(st.src, flags, st.cap, st.null), prev_b, c2, r, out))
            if flags & FIRST and r["cc"] != M.CC_INVALID_OP:
                data_at = len(data)                                    # (a stream that starts afresh: its output begins here)
            c, data = c2, data + out
            if r["status"] == M.DST_FULL:
                queue.insert(0, Step(st.src[r["in_used"]:], 0, resend_caps[k % len(resend_caps)]))
                k += 1
        self.data = data
        # a decode that fails may have written what it decoded before the fault: room for that, and nothing said about those bytes
        self.loose = any(r["cc"] not in (M.CC_OK, M.CC_DATA_LENGTH, M.CC_INVALID_OP) for _, _, _, r, _ in self.calls)
        self.room = len(data) + (80000 if self.loose else 64)


def run_device(eng, scenarios, fmt=None):
    """queue every call of every scenario (round r: call r of the scenarios that have one; the scenarios are ordered by their number
    of calls, so a round is a prefix of the carry array), wait once, compare everything with the model"""
    import torch
    t = torch
    order = sorted(range(len(scenarios)), key=lambda i: -len(scenarios[i].calls))
    sc = [scenarios[i] for i in order]
    n = len(sc)
    fmt = sc[0].fmt if fmt is None else fmt
    rounds = len(sc[0].calls)
    # the device buffers: every call's source, every scenario's outputs end to end, copies of prev for detached windows
    src_at, prev_at, out_at = {}, {}, []
    pos = 16
    chunks = []
    for i, s in enumerate(sc):
        for r, (st, prev_b, _, _, _) in enumerate(s.calls):
            pos = (pos + 15) & ~15
            pos += (i + r) % 16                                        # sources at every alignment
            src_at[i, r] = pos
            chunks.append((pos, st.src))
            pos += len(st.src)
            if s.prev != "contig" and prev_b:
                pos = ((pos + 15) & ~15) + s.prev
                prev_at[i, r] = pos
                chunks.append((pos, prev_b))
                pos += len(prev_b)
    src_h = np.zeros(pos + 64, np.uint8)
    for at, b in chunks:
        src_h[at:at + len(b)] = np.frombuffer(b, np.uint8)
    opos = 16
    for i, s in enumerate(sc):
        opos = ((opos + 15) & ~15) + s.dst_align
        out_at.append(opos)
        opos += s.room
    out_h = np.full(opos + 64, CANARY, np.uint8)
    d_src, d_out = eng.to_device(src_h), eng.to_device(out_h)
    carry_h = np.zeros(n, E.INFLATE_CARRY_DTYPE)
    carry_h.view(np.uint8)[:] = 0xa5                                   # no initial value; phase 0xa5a5a5a5: nothing a call may leave
    carry = eng.to_device(carry_h)
    results, snaps = [], []
    done = [0] * n                                                     # output bytes in front of the call's target
    for r in range(rounds):
        m = sum(1 for s in sc if len(s.calls) > r)
        jobs = np.zeros(m, E.INFLATE_PART_JOB_DTYPE)
        for i in range(m):
            st, prev_b, _, res, out = sc[i].calls[r]
            j = jobs[i]
            j["src"] = 0 if st.null == "src" else d_src.data_ptr() + src_at[i, r]
            j["src_len"] = len(st.src)
            dst = d_out.data_ptr() + out_at[i] + done[i]
            j["dst"] = 0 if st.null == "dst" else dst
            j["dst_cap"] = min(st.cap, sc[i].room - done[i])             # (never beyond the scenario's room; the model's cap where it matters)
            assert j["dst_cap"] == st.cap or (res["status"] != M.DST_FULL and j["dst_cap"] >= len(out))   # (a roomier target than the room left changes nothing)
            j["prev_len"] = len(prev_b) if st.null != "prev" else 5
            j["prev"] = 0 if st.null == "prev" or not prev_b else dst - len(prev_b) if sc[i].prev == "contig" else d_src.data_ptr() + prev_at[i, r]
            j["flags"] = st.flags
            done[i] += len(out)
        rc, res = eng.inflate_stream_parts(fmt, jobs, carry)
        assert rc == 0
        results.append(res)
        snaps.append(carry.clone())
    got_out = d_out.cpu().numpy()                                      # the ONE wait
    done = [0] * n
    for r in range(rounds):
        m = sum(1 for s in sc if len(s.calls) > r)
        res = results[r].cpu().numpy().view(E.INFLATE_PART_RESULT_DTYPE)
        cy = snaps[r].cpu().numpy().view(E.INFLATE_CARRY_DTYPE)
        for i in range(m):
            st, prev_b, c, want, out = sc[i].calls[r]
            what = (sc[i].name, r)
            g = res[i]
            assert (g["cc"], g["status"], g["in_used"], g["out_len"], g["crc"], g["adler"]) == \
                (want["cc"], want["status"], want["in_used"], want["out_len"], want["crc"], want["adler"]), what
            a = out_at[i] + done[i]
            assert got_out[a:a + len(out)].tobytes() == out, what
            done[i] += len(out)
            if c is None:                                              # refused before any FIRST: the record is as it was
                assert cy[i]["phase"] == 0xa5a5a5a5, what
                continue
            k = cy[i]
            assert (k["phase"], k["parts"], k["total_in"], k["total_out"]) == (c["phase"], c["parts"], c["total_in"], c["total_out"]), what
            if c["phase"] == M.HEADER:
                continue
            f = k["frame"]
            assert {x: int(f[x]) for x in M.FRAME_FIELDS} == c["frame"], what
            assert (k["sfbt"], k["rem"], k["dhtlen"], k["subc"], k["crc"], k["adler"]) == (c["sfbt"], c["rem"], c["dhtlen"], c["subc"], c["crc"], c["adler"]), what
            assert k["tail_len"] == len(c["tail"]) and k["tail"][:len(c["tail"])].tobytes() == c["tail"], what
            if c["sfbt"] & 0xe == 0xc:
                nb = (c["dhtlen"] + 7) // 8
                assert k["dht"][:nb].tobytes() == c["dht"][:nb], what
    # nothing beyond what the model wrote: the outputs end to end, canaries everywhere else
    want_out = np.full(len(out_h), CANARY, np.uint8)
    for i, s in enumerate(sc):
        want_out[out_at[i]:out_at[i] + len(s.data)] = np.frombuffer(s.data, np.uint8)
        if s.loose:
            a, b = out_at[i] + len(s.data), out_at[i] + s.room
            want_out[a:b] = got_out[a:b]
    assert np.array_equal(got_out, want_out)


def two_part_scenarios(fmt, body_samples=2):
    out = []
    for s in STREAMS:
        _, z = framed(s, fmt)
        for k in two_part_cuts(s, fmt, body_samples=body_samples):
            out.append(Scenario(fmt, [Step(z[:k]), Step(z[k:] + b"beyond")], name="%s@%d" % (s.name, k)))
    return out


@pytest.mark.parametrize("fmt", [RAW, ZLIB, GZIP])
def test_two_parts(eng, fmt):
    sc = two_part_scenarios(fmt)
    assert all(s.data == BY_NAME[s.name.split("@")[0]].data and s.calls[-1][3]["status"] == M.S_DONE for s in sc)
    run_device(eng, sc)


@pytest.mark.parametrize("fmt", [RAW, ZLIB, GZIP])
def test_many_parts_one_wait(eng, fmt):
    rnd = random.Random(17)
    sc = []
    for s in STREAMS:
        _, z = framed(s, fmt)
        for _ in range(4):
            sc.append(Scenario(fmt, [Step(p) for p in many_part_splits(z, rnd)], name=s.name + "/split"))
        sc.append(Scenario(fmt, [Step(p) for p in byte_parts(z)], name=s.name + "/bytes"))
    assert all(s.data == BY_NAME[s.name.split("/")[0]].data for s in sc)
    run_device(eng, sc)


def test_gzip_header_cut_at_every_byte(eng):
    s = BY_NAME["fixed"]
    head = F.gzip_header(flg=F.FEXTRA | F.FNAME | F.FCOMMENT | F.FHCRC, mtime=0x12345678, xfl=2, os_=3, extra=b"ab\x02\x00xy", name=b"a name",
                         comment=b"a comment")
    z = head + s.comp + struct.pack("<II", zlib.crc32(s.data), len(s.data))
    sc = [Scenario(GZIP, [Step(z[:k]), Step(z[k:])], name="hdr@%d" % k) for k in range(1, len(head) + 2)]
    sc.append(Scenario(GZIP, [Step(z[i:i + 1]) for i in range(len(head) + 3)] + [Step(z[len(head) + 3:])], name="hdr/bytes"))
    bad = F.gzip_header(flg=F.FNAME | F.FHCRC, name=b"x", hcrc_ok=False)
    sc.append(Scenario(GZIP, [Step(bad[:5]), Step(bad[5:] + s.comp)], name="bad hcrc"))
    assert sc[0].calls[-1][2]["frame"]["name_off"] == 10 + 2 + 6 and sc[-1].calls[-1][2]["frame"]["status"] == F.BAD_HCRC
    run_device(eng, sc)
    # zlib FDICT: NEED_DICT with dictid set, nothing decoded, phase failed -- the six bytes in one part, and cut
    zd = b"\x78\xbb" + struct.pack(">I", 0xcafef00d) + s.comp
    sc = [Scenario(ZLIB, [Step(zd[:k]), Step(zd[k:])], name="fdict@%d" % k) for k in range(1, 7)] + [Scenario(ZLIB, [Step(zd)], name="fdict")]
    for x in sc:
        c, r = x.calls[-1][2], x.calls[-1][3]
        assert c["frame"]["status"] == F.NEED_DICT and c["frame"]["dictid"] == 0xcafef00d and c["phase"] == M.FAILED and x.data == b""
    run_device(eng, sc)
    # AUTO: gzip by its magic, zlib else, cut between the two bytes that say so
    _, zz = framed(s, ZLIB)
    sc = [Scenario(AUTO, [Step(z[:1]), Step(z[1:])], name="auto gzip"), Scenario(AUTO, [Step(zz[:1]), Step(zz[1:])], name="auto zlib")]
    assert all(x.data == s.data for x in sc)
    run_device(eng, sc, AUTO)


@pytest.mark.parametrize("fmt", [RAW, ZLIB, GZIP])
def test_full_targets(eng, fmt):
    rnd = random.Random(19)
    sc = []
    for s in STREAMS:
        head, z = framed(s, fmt)
        for _ in range(6):
            k = rnd.randrange(len(head) + 1, len(z))
            small = rnd.randrange(1, min(3000, len(s.data) // 8))
            caps = [rnd.randrange(1, 600), rnd.randrange(300, 70000), BIG]
            sc.append(Scenario(fmt, [Step(z[:k], cap=small), Step(z[k:], cap=rnd.randrange(1, 5000))], whole=s.comp, resend_caps=caps, name=s.name))
            # ... and a target of one or two bytes behind a cut inside a token: it fills inside the old tail when that token is a match
            k = rnd.randrange(len(head) + 1, len(z))
            sc.append(Scenario(fmt, [Step(z[:k]), Step(z[k:], cap=rnd.choice([1, 2]))], whole=s.comp, resend_caps=caps, name=s.name))
    assert all(x.data == BY_NAME[x.name].data for x in sc)
    full = [r for x in sc for _, _, _, r, _ in x.calls if r["status"] == M.DST_FULL]
    assert len(full) > len(sc) and any(r["in_used"] == 0 for r in full)    # ... caps that fill inside the old tail among them
    run_device(eng, sc)


def test_windows_and_alignments(eng):
    sc = []
    for s in (BY_NAME["dynamic"], BY_NAME["mixed"], BY_NAME["own"]):
        _, z = framed(s, ZLIB)
        k = len(z) * 2 // 3
        for prev in ("contig", 0, 1, 15):
            for dst_align in (0, 1, 15):
                sc.append(Scenario(ZLIB, [Step(z[:k]), Step(z[k:])], prev=prev, keep=32768, dst_align=dst_align, name=s.name))
        # a window shorter than a match reaches: the oracle's verdict for the same history
        for keep in (0, 1, 100, 4096):
            sc.append(Scenario(ZLIB, [Step(z[:k]), Step(z[k:])], prev=1, keep=keep, name=s.name + "/short"))
    good = [x for x in sc if "/" not in x.name]
    assert all(x.data == BY_NAME[x.name].data for x in good)
    assert any(x.calls[-1][3]["status"] == M.S_FAILED and x.calls[-1][2]["frame"]["status"] == F.DEFLATE for x in sc if "/" in x.name)
    run_device(eng, sc)


def test_damage(eng):
    s, s2 = BY_NAME["dynamic"], BY_NAME["fixed"]
    _, zl = framed(s, ZLIB)
    _, gz = framed(s, GZIP)
    _, gz2 = framed(s2, GZIP)
    k = len(zl) // 2
    sc = []
    # a bad distance in part 2: the first match of a stream behind a window that is not handed over
    sc.append(Scenario(ZLIB, [Step(zl[:k]), Step(zl[k:], prev_len=0)], name="bad distance"))
    assert sc[-1].calls[-1][3]["status"] == M.S_FAILED and sc[-1].calls[-1][3]["cc"] not in (0, 3)
    # a wrong Adler-32, CRC-32 and ISIZE, the trailer split over two parts
    bad = bytearray(zl); bad[-1] ^= 1
    sc.append(Scenario(ZLIB, [Step(bytes(bad[:-2])), Step(bytes(bad[-2:]))], name="adler"))
    bad = bytearray(gz); bad[-6] ^= 1
    sc.append(Scenario(GZIP, [Step(bytes(bad[:-7])), Step(bytes(bad[-7:]) + b"more")], name="crc"))
    bad = bytearray(gz); bad[-1] ^= 0x40
    sc.append(Scenario(GZIP, [Step(bytes(bad[:-3])), Step(bytes(bad[-3:]))], name="isize"))
    assert [x.calls[-1][2]["frame"]["status"] for x in sc[1:]] == [F.BAD_CHECK, F.BAD_CHECK, F.BAD_LENGTH]
    # bytes behind the trailer; a second member behind it: DONE, in_used points at the member
    sc.append(Scenario(GZIP, [Step(gz[:k]), Step(gz[k:] + gz2)], name="second member"))
    assert sc[-1].calls[-1][3]["status"] == M.S_DONE and sc[-1].calls[-1][3]["in_used"] == len(gz) - k
    # a part sent to a done carry without FIRST: refused, the carry unchanged; FIRST on a used carry starts afresh
    sc.append(Scenario(GZIP, [Step(gz), Step(gz2, flags=0), Step(gz2[:30], flags=FIRST), Step(gz2[30:], flags=0)], name="done, then afresh"))
    x = sc[-1]
    assert x.calls[1][3]["cc"] == M.CC_INVALID_OP and x.calls[1][2] is x.calls[0][2] and x.data == s.data + s2.data
    # the other refusals, between good neighbours; a failed stream that goes on being sent is refused
    sc.append(Scenario(GZIP, [Step(gz[:k]), Step(gz[k:], null="src"), Step(gz[k:], null="dst"), Step(gz[k:], flags=4), Step(gz[k:], null="prev"),
                              Step(gz[k:], flags=FIRST, prev_len=16), Step(gz[k:])], name="refusals"))
    assert sc[-1].data == s.data and [c[3]["cc"] for c in sc[-1].calls[1:6]] == [M.CC_INVALID_OP] * 5
    sc.append(Scenario(ZLIB, [Step(b"\x78\x9d" + s.comp), Step(s.comp)], name="bad header, then refused"))
    assert sc[-1].calls[0][2]["frame"]["status"] == F.BAD_HEADER and sc[-1].calls[1][3]["cc"] == M.CC_INVALID_OP
    for fmt in (ZLIB, GZIP):
        run_device(eng, [x for x in sc if x.fmt == fmt])


def test_whole_stream_in_one_first_part_is_the_framed_call(eng):
    import torch
    for fmt in (ZLIB, GZIP):
        zs = [framed(s, fmt)[1] + b"tail" for s in STREAMS]
        run_device(eng, [Scenario(fmt, [Step(z)], name=s.name) for s, z in zip(STREAMS, zs)])
        # ... and the framed call on the same bytes says the same (the model already did)
        stride_in, stride_out = 72 << 10, 72 << 10
        host = np.zeros((len(zs), stride_in), np.uint8)
        for i, z in enumerate(zs):
            host[i, :len(z)] = np.frombuffer(z, np.uint8)
        src = torch.from_numpy(host).to(eng.dev)
        dst = torch.zeros((len(zs), stride_out), dtype=torch.uint8, device=eng.dev)
        jobs = eng.jobs_strided(src, stride_in, np.array([len(z) for z in zs], np.uint32), dst, stride_out, stride_out)
        res, frames = eng.decompress_framed(fmt, jobs, len(zs))
        r, f = eng.results_to_host(res), eng.results_to_host(frames, E.FRAME_DTYPE)
        out = dst.cpu().numpy()
        for i, (s, z) in enumerate(zip(STREAMS, zs)):
            c, want, _ = M.part(None, fmt, z, BIG, b"", FIRST)
            assert out[i, :r["tpbc"][i]].tobytes() == s.data and r["tpbc"][i] == want["out_len"]
            assert (r["crc"][i], r["adler"][i]) == (want["crc"], want["adler"]) and f["end"][i] == want["in_used"]
            assert {x: int(f[x][i]) for x in M.FRAME_FIELDS} == c["frame"], s.name


def with_env(env, fn):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        fn()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def test_chunking_does_not_show(eng):
    """the scratch knob at a value that forces several chunks, with one stream larger than it: the model's answer all the same"""
    rnd = random.Random(23)
    sc = []
    for s in STREAMS:
        _, z = framed(s, ZLIB)
        sc.append(Scenario(ZLIB, [Step(p) for p in many_part_splits(z, rnd)], name=s.name))
    run_device(eng, sc)
    with_env({"NXZ_INFLATE_PART_SCRATCH": "50000"}, lambda: run_device(eng, sc))      # (the stored stream's parts are larger)
    with_env({"NXZ_INFLATE_PART_SCRATCH": "1"}, lambda: run_device(eng, sc))          # a chunk a stream


@pytest.mark.parametrize("fmt", [RAW, ZLIB, GZIP])
@pytest.mark.parametrize("env", [{"NXZ_INFLATE_LANES_MIN": "1"}, {"NXZ_INFLATE_WG": "0"}], ids=["lanes_min_1", "wg_0"])
def test_two_parts_on_other_routes(eng, env, fmt):
    """the two-part family again, every framing and every cut, under the knobs that name another decode route"""
    sc = two_part_scenarios(fmt)
    with_env(env, lambda: run_device(eng, sc))
