"""What the blocks of tests/compress_edge_cases.py cover, by the oracle alone (no GPU): tests/test_gpu_compress_edges.py part A
runs them on the device with targets around the exact length, and cannot lose one of these classes without this test failing."""
import zlib

import pytest

import compress_edge_cases as E


@pytest.mark.parametrize("emitter", list(E.EMITTERS))
def test_every_emitter_has_the_coverage(emitter):
    form, cls, env, through_dict = E.EMITTERS[emitter]
    cs = E.cases(cls)
    assert all(c.exp is not None for c in cs)                     # the canned table codes every symbol of its blocks
    v = E.coverage(cs)
    assert v["sizes"] >= set(E.SIZES)
    assert v["mod4"] == {0, 1, 2, 3}
    assert v["straddle"] >= 1                                     # (bits in front of the end-of-block code) % 32 + its length > 32
    assert v["dword_exact"] >= 1                                  # the block's last bit is a dword's last bit
    assert len(v["empty_header_bits"]) == 1
    if E.CLASSES[cls][0] != "fixed":                              # an empty block whose header alone is longer than a dword
        assert v["empty_header_bits"][0] > 32
    # more bytes out than in (cc 64) wherever the history, which counts as input, leaves room for it
    assert {c.cc for c in cs} == ({0, 64} if len(E.history(cls)) <= 16 else {0})


def test_the_emitters_are_the_issue_s():
    assert set(E.EMITTERS) == {"FHT", "FHT_COUNT", "RESUME_FHT/16", "RESUME_FHT/32768", "DHT", "DHTGEN", "DHTGEN_COUNT", "DHTGEN/fused",
                               "DHTGEN/dict"}
    assert len(E.history("fixed/16")) == 16 and len(E.history("fixed/32768")) == 32768 and len(E.history("own/dict")) == 992
    assert E.EMITTERS["DHTGEN/fused"][2] == {"NXZ_FUSED_GEN": "1"}


@pytest.mark.parametrize("cls", list(E.CLASSES))
def test_expected_blocks_inflate_and_caps_are_the_rule_s(cls):
    for c in E.cases(cls):
        z = zlib.decompressobj(-15, zdict=c.hist) if c.hist else zlib.decompressobj(-15)
        assert z.decompress(c.exp) == c.body and z.eof, c.name
        caps, L = c.caps(), c.L
        assert set(caps) == {x for x in (0, 1, 3, 4, L - 5, L - 4, L - 3, L - 2, L - 1, L, L + 1, L + 2, L + 3, L + 4, L & ~3, (L & ~3) + 4)
                             if x >= 0}
        assert any(x < L for x in caps) and any(x >= L for x in caps) and any(x % 4 for x in caps)
