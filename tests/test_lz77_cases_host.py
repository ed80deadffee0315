"""The edge-case set of tests/lz77_cases.py on the CPU: a census (the set reaches the regimes and edges it was written for, by the
oracle's own tap and token stream), sensitivity (the oracle built with one constant changed gives other tokens on the family
written for that constant -- so a kernel with that constant wrong cannot pass tests/test_gpu_lz77_edges.py), and RFC validity
(system zlib inflates every block's oracle output, fixed and own-table, to the input)."""
import os
import subprocess
import zlib

import pytest

import lz77_cases as Z
import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = Z.TILE


@pytest.fixture(scope="module")
def parsed():
    """name -> (data, hist, events, (text, first tile's tokens, use_second, lazy_max)); the oracle runs once per case"""
    out = {}
    for name, data, hist in Z.all_cases():
        tok, nt, regime = O.lz77_regime(data, hist)
        out[name] = (data, hist, Z.events(tok, nt), regime[0], bytes(tok)[:4 * nt])
    return out


def token_at(ev, at):
    return next(e for e in ev if e[0] <= at < e[0] + e[1])


def test_generators_are_deterministic():
    Z.all_cases.cache_clear()
    Z.token_threshold.cache_clear()
    a = Z.all_cases()
    Z.all_cases.cache_clear()
    Z.token_threshold.cache_clear()
    assert a == Z.all_cases()
    assert all(h <= 32768 and len(d) <= 65536 for _, d, h in a)


def test_census(parsed):
    later = lambda n: n > TILE
    regimes = {(r[0], int(r[1] >= 3072)) for d, h, ev, r, _ in parsed.values() if later(len(d) - h)}
    assert regimes == {(0, 0), (0, 1), (1, 0), (1, 1)}, regimes
    # second entries and the lazy step live behind the first tile: not text, hard, later tiles
    live = [n for n, (d, h, ev, r, _) in parsed.items() if later(len(d) - h) and r[2] == 1 and r[3] == 32]
    assert len(live) >= 8 and any(n.startswith("bin-hard") for n in live), live
    assert all(parsed[n][3][0] == 0 and parsed[n][3][1] >= 3072 for n in live)
    deep = sum(1 for n in live for p, l, dist in parsed[n][2] if p >= TILE and dist > 1)
    assert deep >= 2000, deep
    per_block = [sum(1 for p, l, dist in parsed[n][2] if p >= TILE and dist > 1) for n in live if n.startswith("bin-hard/65536")]
    assert min(per_block) >= 2000, per_block
    # the two thresholds, from both sides
    for tag, regs in (("high", {3071: (0, 0, 32), 3072: (0, 1, 32), 3073: (0, 1, 32)}),
                      ("text", {3071: (1, 0, 32), 3072: (1, 0, 0), 3073: (1, 0, 0)})):
        for t0, (text, second, lazy) in regs.items():
            assert parsed["threshold/%s/%d" % (tag, t0)][3] == (text, t0, second, lazy)
    for name, (d, h, ev, r, _) in parsed.items():
        if name.startswith("text-threshold"):
            m = Z.META[name]
            assert sum(b >> 7 for b in d[:m["t0n"]]) == m["high"]
            assert r[0] == int(m["high"] * 16 < m["t0n"]) and r[1] >= 3072, (name, r)
    assert parsed["text-threshold/32768/1023"][3][2:] == (0, 0) and parsed["text-threshold/32768/1024"][3][2:] == (1, 32)
    assert parsed["text-threshold/8000/499"][3][0] == 1 and parsed["text-threshold/8000/500"][3][0] == 0
    # the window's edge, inside the block and from the history
    for where in ("block", "history"):
        for dist in (32767, 32768):
            ev = parsed["window/%s/%d" % (where, dist)][2]
            assert token_at(ev, Z.META["window/%s/%d" % (where, dist)]["marker"])[1:] == (24, dist)
        name = "window/%s/32769" % where
        ev, at = parsed[name][2], Z.META[name]["marker"]
        assert all(token_at(ev, at + i) == (at + i, 1, 0) for i in range(24)), name
    assert all(dist <= 32768 for v in parsed.values() for _, _, dist in v[2])
    for period in (1, 2, 3, 4, 8):
        ev = parsed["window/period/%d" % period][2]
        assert {dist for _, _, dist in ev if dist} == {period}
    # lazy: k < 32 gives way to the longer match one byte on, k >= 32 does not
    for where in ("tile0", "tile1"):
        for k in (30, 31, 32, 33):
            name = "lazy/%s/%d" % (where, k)
            ev, at = parsed[name][2], Z.META[name]["at"]
            if k < 32:
                assert token_at(ev, at) == (at, 1, 0) and token_at(ev, at + 1)[:2] == (at + 1, k + 11), name
            else:
                assert token_at(ev, at)[:2] == (at, k), name
    # matches cut at a tile's end: 3 bytes are a match, 2 are not
    for rem in (0, 1, 2, 3, 4, 61, 62, 63):
        name = "cut/tile/%d" % rem
        ev, at = parsed[name][2], Z.META[name]["at"]
        want = (at, 64 - rem, at - 50) if 64 - rem >= 3 else (at, 1, 0)
        assert token_at(ev, at) == want, (name, token_at(ev, at))
        assert not any(p < TILE < p + l for p, l, _ in ev), name          # no token crosses a tile's end
    assert token_at(parsed["cut/tile/61"][2], TILE - 3) == (TILE - 3, 3, TILE - 3 - 50)
    for rem in (1, 2, 3, 4, 5):
        ev = parsed["cut/last-tile/%d" % rem][2]
        assert token_at(ev, TILE - 30)[:2] == (TILE - 30, 30)
        assert token_at(ev, TILE) == ((TILE, rem, TILE - 30 - 50) if rem >= 4 else (TILE, 1, 0)), rem
    for n in (20000, 65536):
        for left in (5, 4, 3, 2):
            name = "cut/end/%d/%d" % (n, left)
            tok = token_at(parsed[name][2], n - left)
            assert tok[:2] == ((n - left, left) if left >= 4 else (n - left, 1)), (name, tok)
    # the longest match
    lengths = {l for v in parsed.values() for _, l, _ in v[2]}
    assert {3, 257, 258} <= lengths and max(lengths) == 258
    for L in (257, 258, 259, 516, 517):
        for kind, dist_of in (("far", lambda m: m["L"] + 100), ("run", lambda m: 1)):
            name = "length/%s/%d" % (kind, L)
            m = Z.META[name]
            ev, at = parsed[name][2], m["at"] + (kind == "run")
            assert token_at(ev, at) == (at, min(L, 258), dist_of(m)), (name, token_at(ev, at))
            if L > 258 + 2:                                       # the rest at the same distance (the segment parse may cut it in two)
                assert all(token_at(ev, q)[2] == dist_of(m) for q in range(at + 258, at + L)), name
    for m in (4, 5):
        at = Z.META["length/tie/%d" % m]["at"]
        assert token_at(parsed["length/tie/%d" % m][2], at) == (at, m, 1)
    # deep in a run: from 12 equal bytes on, neither inserted nor looked up
    for name, (d, h, ev, r, _) in parsed.items():
        if name.startswith("run/"):
            m = Z.META[name]
            assert (token_at(ev, m["at"]) == (m["at"], 16, m["far"])) == (not m["deep"]), (name, token_at(ev, m["at"]))
        if name.startswith("piece/"):
            m = Z.META[name]
            want = (m["at"], 16, m["far"]) if m["visible"] else (m["at"], 5, m["near"])
            assert token_at(ev, m["at"]) == want, (name, token_at(ev, m["at"]))
    # every history length class, with matches that reach into the history
    for tag in ("bin", "text"):
        for hl in Z.HISTORIES:
            d, h, ev, r, _ = parsed["history/%s/%d" % (tag, hl)]
            assert h == hl and r[1] >= 3072 and r[0] == (tag == "text")
            assert hl < 4 or any(dist > p for p, _, dist in ev)


MUTANTS = [("NXO_SECOND_MIN_TOKENS", 3071, "threshold/"), ("NXO_SECOND_MIN_TOKENS", 3073, "threshold/"),
           ("NXO_TEXT_HIGH_DIV", 15, "text-threshold/"), ("NXO_TEXT_HIGH_DIV", 17, "text-threshold/"),
           ("NXO_LAZY_MAX", 31, "lazy/"), ("NXO_LAZY_MAX", 33, "lazy/"),
           ("NXO_PIECE", 256, "piece/"), ("NXO_PIECE", 1024, "piece/"),
           ("NXO_CHUNK", 32, "window/period/"), ("NXO_CHUNK", 128, "window/period/"),
           ("NXO_RLE", 0, "length/run/"),
           ("NXO_CAND_WINDOW", 32767, "window/"), ("NXO_MAXMATCH", 257, "length/"), ("NXO_DEEP_RUN", 11, "run/")]
# what exactly each change must flip (and nothing else of its family): the pairs the families were built as
KILLS_ONLY = {("NXO_SECOND_MIN_TOKENS", 3071): {"threshold/high/3071", "threshold/text/3071"},
              ("NXO_SECOND_MIN_TOKENS", 3073): {"threshold/high/3072", "threshold/text/3072"},
              ("NXO_TEXT_HIGH_DIV", 17): {"text-threshold/32768/1023", "text-threshold/20000/1023", "text-threshold/32768/964"},
              ("NXO_TEXT_HIGH_DIV", 15): {"text-threshold/32768/1024", "text-threshold/20000/1024", "text-threshold/32768/1092"},
              ("NXO_LAZY_MAX", 31): {"lazy/tile0/31", "lazy/tile1/31"},
              ("NXO_LAZY_MAX", 33): {"lazy/tile0/32", "lazy/tile1/32"},
              ("NXO_CAND_WINDOW", 32767): {"window/block/32768", "window/history/32768"}}


@pytest.mark.parametrize("macro,value,fam", MUTANTS, ids=["%s=%d" % m[:2] for m in MUTANTS])
def test_sensitivity(parsed, tmp_path, macro, value, fam):
    """oracle/nxz_lz77.c with one constant changed parses at least one case of the family written for that constant differently.
    Every mutant of the list is killed; where the family was built as pairs around the constant, exactly the expected side flips."""
    so = str(tmp_path / "mutant.so")
    subprocess.run(["gcc", "-O1", "-fPIC", "-shared", "-std=gnu11", "-D%s=%d" % (macro, value), "-o", so,
                    os.path.join(ROOT, "oracle", "nxz_lz77.c"), os.path.join(ROOT, "oracle", "nxz_huff.c")], check=True)
    L = O.load_variant(so)
    killed = set()
    for name, (data, hist, ev, r, raw) in parsed.items():
        if name.startswith(fam):
            tok, nt = O.lz77(data, hist, L)
            if bytes(tok)[:4 * nt] != raw:
                killed.add(name)
    print(macro, value, sorted(killed))
    assert killed, (macro, value)
    if (macro, value) in KILLS_ONLY:
        assert killed == KILLS_ONLY[(macro, value)], killed


def test_every_block_inflates_with_zlib(parsed):
    for name, (data, hist, ev, r, _) in parsed.items():
        fixed, bits = O.deflate_fixed(data, hist)
        tok, nt = O.lz77(data, hist)
        ll, d = O.counts(tok, nt)
        dht, dhtlen = O.dhtgen(ll, d)
        own, obits = O.deflate_dynamic(data, dht, dhtlen, hist)
        assert own is not None, name
        for stream in (fixed, own):
            z = zlib.decompressobj(-15, zdict=data[:hist]) if hist else zlib.decompressobj(-15)
            assert z.decompress(stream) == data[hist:] and z.eof, name
