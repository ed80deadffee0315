"""The resume cases of tests/resume_cases.py, with the oracle alone: the set holds what the GPU tests rely on, and every
expected result is independent of the cut -- oracle part 1 + oracle part 2 is the oracle in one go."""
import zlib

import oracle_lib as O
import resume_cases as R


def test_block_starts_are_block_starts():
    for s in R.streams():
        out, st = O.inflate(s.comp, R.CAP_MAX)
        assert st.err == 0 and st.final_eob and st.out_subc < 8 and out == s.data, s.name
        assert len(s.data) <= 70000
        if s.starts is None:                                                              # (found by the oracle, cut by cut)
            continue
        for h in s.starts[1:]:
            _, st = O.inflate(s.comp[:h], R.CAP_MAX)
            assert st.err == 0 and st.out_sfbt == 0xe and st.out_subc == 0, (s.name, h)      # at a header, on a byte boundary
        for h in s.starts:                                                                # the bands end behind the header
            e = R.header_end(s, h)
            _, st = O.inflate(s.comp[:e], R.CAP_MAX)
            # (inside the block -- or, behind an empty stored block, at the next header)
            assert (st.out_sfbt & 0xe) in (0x8, 0xa, 0xc) or (st.out_sfbt, st.out_subc) == (0xe, 0), (s.name, h, e)


def test_the_set_covers_what_the_issue_names():
    cs = R.cases()
    assert len(cs) <= 800
    kinds = {}
    for c in cs:
        kinds.setdefault(c.sfbt & 0xe, []).append(c)
    assert set(kinds) == set(R.KINDS)
    for kind, v in kinds.items():
        assert {c.sfbt & 1 for c in v} == {0, 1}, hex(kind)                               # BFINAL 0 and 1
        assert any(c.m == 0 for c in v), hex(kind)                                        # an empty part 2
        assert any(c.m > 0 and c.err == 0 and not c.final_eob for c in v), hex(kind)      # suspends again in part 2
    for kind in (0xa, 0xc, 0xe):
        assert {c.subc for c in kinds[kind]} == set(range(8)), hex(kind)
    assert all(c.subc == 0 and c.rem for c in kinds[0x8]) and all(c.rem == 0 for c in cs if (c.sfbt & 0xe) != 0x8)
    rems = {c.rem for c in kinds[0x8]}
    assert 1 in rems and 65535 in rems
    assert any(c.rem < len(c.part2) for c in kinds[0x8])                                  # the block ends inside part 2
    assert any(c.subc1 > 7 for c in kinds[0xe])                                           # a stop inside a table
    aligned = [c for c in kinds[0xc] if c.layout == "b" and (c.pad + len(c.hist)) % 16 == 0]
    assert sum(len(c.part2) >= 2048 for c in aligned) >= 20
    assert sum(len(c.part2) >= 4096 for c in aligned) >= 5
    assert {c.err for c in cs} <= {0, 13, 67}
    assert {c.layout for c in cs} == {"a", "b", "c"}
    assert len({c.shift for c in cs if c.layout == "a"}) == 16                            # the stream at every alignment
    assert any(c.err == 67 for c in cs if c.layout == "c") and any(c.err == 0 and c.tpbc for c in cs if c.layout == "c")
    short = [c for c in cs if c.err == 13]
    assert len(cs) // 20 <= len(short) <= len(cs) // 5                                    # about a tenth: a target one byte short
    assert all(len(c.hist) <= 32768 and len(c.pad * b"0") < 16 for c in cs)
    assert sum(c.cap + 64 for c in cs) < 48 << 20                                         # the targets, all told


def test_every_case_is_the_oracle_in_one_go():
    comp = {s.name: s.comp + R.TRAILER for s in R.streams()}
    whole = {}
    for c in R.cases():
        if c.err or c.m == 0:                  # (an empty part 2 leaves out the byte the stream stands in: the oracle's answer is all there is)
            continue
        key = (c.stream, c.pos + c.m)
        if key not in whole:
            whole[key] = O.inflate(comp[c.stream][:c.pos + c.m], R.CAP_MAX)
        out, st = whole[key]
        assert st.err == 0
        n1 = len(out) - c.tpbc
        assert n1 >= 0 and out[n1:] == c.out, (c.stream, c.k, c.m)
        assert zlib.crc32(out[:n1]) == c.crc1 and zlib.adler32(out[:n1]) == c.adler1
        if c.layout != "c":
            assert out[:n1][-32768:] == c.hist
        assert zlib.crc32(c.out, c.crc1) == zlib.crc32(out) and zlib.adler32(c.out, c.adler1) == zlib.adler32(out)
        assert (st.out_sfbt, st.out_subc, bool(st.final_eob)) == (c.out_sfbt, c.out_subc, c.final_eob), (c.stream, c.k, c.m)
        if (st.out_sfbt & 0xe) == 0x8:
            assert st.out_rembytecnt == c.out_rem
        if (st.out_sfbt & 0xe) == 0xc:
            nb = (st.out_dhtlen + 7) // 8
            assert st.out_dhtlen == c.out_dhtlen and bytes(st.out_dht)[:nb] == c.out_dht[:nb]


def test_a_job_inside_a_dynamic_block_without_a_table_is_cc68():
    out, st = O.inflate(b"\x00" * 16, 100, sfbt=0xc)
    assert st.err == 68 and st.tpbc == 0
    out, st = O.inflate(b"\x00" * 16, 100, sfbt=0xd, dhtlen=100)                          # (no table, whatever its length says)
    assert st.err == 68 and st.tpbc == 0
