"""The hand-built streams of tests/deflate_handmade.py, with the oracle and system zlib alone (no GPU): the set holds what
the kernel tests rely on, and the oracle is held to zlib wherever zlib has a verdict -- an end of stream in zlib is an end
of stream with the same bytes in the oracle, an error in the oracle is an error in zlib.  The two places where the oracle
is more lenient on purpose are named here, one by one: a change of either rule shows as a changed set."""
import zlib

import deflate_handmade as H
import oracle_lib as O

# an incomplete code is no error by itself (oracle/nxz_huff.c refuses over-subscribed codes only; zlib refuses the header)
LENIENT = {
    "lenient/an-incomplete-literal-length-code-of-which-only-assigned-codes-are-used",
    "lenient/an-incomplete-distance-code-of-which-only-assigned-codes-are-used",
    "lenient/an-incomplete-code-length-code-of-which-only-assigned-codes-are-used",
}
# a code that no symbol has, in the last bits of the source with fewer bits behind it than the longest code: the oracle
# suspends (more source may follow), zlib fails at once.  With 8 bytes behind the same bits both fail ("/padded").
SUSPENDS = {"error/%s/at-the-end" % n for n in (
    "fixed-code-distance-symbol-30", "fixed-code-distance-symbol-31", "use-of-an-unassigned-literal-length-code",
    "use-of-an-unassigned-distance-code", "use-of-an-unassigned-code-length-code", "a-match-in-a-block-with-no-distance-code")}


def test_the_oracle_against_zlib_case_by_case():
    lenient, suspends = set(), set()
    for r in H.records():
        verdict, out = H.zlib_verdict(r.src, r.hist, r.cap)
        if verdict == "end":
            assert r.err == 0 and r.final_eob and r.out == out, r.name
        if r.err == 13:                                    # (zlib has no such error: it stands with the capacity full and more to come)
            assert verdict == "more" and len(out) == r.cap + 1, r.name
        elif r.err:
            assert r.err in (66, 67, 68) and verdict == "error", (r.name, r.err, verdict)
        elif verdict == "error":
            (lenient if r.final_eob else suspends).add(r.name)
        if r.family == "valid":
            assert verdict == "end" and r.out_subc < 8, r.name
        assert r.tpbc <= r.cap and len(r.out) == r.tpbc, r.name
    assert lenient == LENIENT
    assert suspends == SUSPENDS


def test_the_set_holds_what_the_kernel_tests_rely_on():
    recs = H.records()
    assert 120 <= len(recs) <= 200
    by = {f: [r for r in recs if r.family == f] for f in H.FAMILIES}
    assert all(by[f] for f in H.FAMILIES) and sum(len(v) for v in by.values()) == len(recs)
    assert {r.err for r in recs} == {0, 13, 66, 67, 68}
    # every output but one fits 40 KiB; that one is the stored block of 65535 bytes
    assert [r.name for r in recs if r.tpbc > 40 * 1024 and r.family != "target"] == ["valid/a-stored-block-of-length-65535-between-huffman-blocks"]
    assert all(r.cap == r.tpbc and r.final_eob and not r.err for r in by["valid"] + by["lenient"])
    assert all(r.cap == H.CAP_REST for r in by["error"] + by["target"] + by["cut"])
    assert all(r.err == 13 for r in by["target"])
    # errors: in the first block with nothing and with 8 bytes behind them, and in the third block behind 30 KiB of output
    names = sorted({r.name.split("/")[1] for r in by["error"]})
    assert len(names) >= 20
    for n in names:
        at_end, padded, third = (next(r for r in by["error"] if r.name == "error/%s/%s" % (n, p)) for p in ("at-the-end", "padded", "third-block"))
        assert padded.err in (66, 67, 68) and padded.src == at_end.src + bytes(8), n
        assert at_end.err in (0, padded.err) and (at_end.err or not at_end.final_eob), n
        assert third.err == padded.err and third.tpbc >= H.GOOD and padded.tpbc < 4, n
        assert (at_end.err == 0) == (at_end.name in SUSPENDS), n
    # cuts: every kind of place, every one a suspension where the kind says
    for kind in H.CUT_KINDS:
        v = [r for r in by["cut"] if r.name.split("/")[1] == kind]
        assert v, kind
        for r in v:
            assert r.err == 0 and not r.final_eob, r.name
            inside = (r.out_sfbt & 0xe) == 0xe if kind != "length-and-distance" else (r.out_sfbt & 0xe) in (0xa, 0xc)
            assert inside and r.out_subc > 0, (r.name, hex(r.out_sfbt))
    # where a job stops that does not end: at a header, in a fixed and in a dynamic block (its table handed back)
    assert {r.out_sfbt & 0xe for r in recs if not r.err and not r.final_eob} == {0xa, 0xc, 0xe}
    assert any(r.out_dhtlen for r in recs if (r.out_sfbt & 0xe) == 0xc)
    hists = {len(r.hist) for r in recs}
    assert {0, 1, 100, 32768} <= hists
    assert sum(r.cap + 64 + len(r.hist) + len(r.src) for r in recs) < 8 << 20


def test_the_tables_of_15_bits_are_what_they_say():
    import ctypes as C
    ll, dd = H.hand_lengths()
    dht, dhtlen = H.hand_table()
    codes = O.Codes()
    assert O.lib().nxo_dht_parse(dht, dhtlen, C.byref(codes)) == dhtlen
    assert list(codes.ll_len)[:286] == ll and list(codes.d_len)[:30] == dd
    assert max(ll) == 15 and max(dd) == 15 and H.kraft(ll) == 1.0 and H.kraft(dd) == 1.0
    long_ones = [r for r in H.records() if "15-bit" in r.name or "fibonacci" in r.name]
    assert len(long_ones) == 3
    for r in long_ones:
        assert zlib.decompressobj(-15, zdict=r.hist).decompress(r.src) == r.out if r.hist else zlib.decompressobj(-15).decompress(r.src) == r.out
    last = next(r for r in H.records() if r.name == "valid/a-block-whose-longest-code-ends-in-the-last-bit-of-the-source")
    assert last.out_subc == 0 and last.final_eob
    _, st = O.inflate(last.src[:-1], 100)                  # the 15 bits of its end-of-block are its last
    assert st.err == 0 and not st.final_eob and st.out_subc == 15 - 8
