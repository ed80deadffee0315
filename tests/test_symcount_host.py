"""The arithmetic of nxzsc::count_kernel (power-gzip_amd/csrc/nxz_symcount.h: the length and distance symbols, a lane's share
of a round, the masks for what lies behind the block) compiled for the host under AddressSanitizer and UBSan
(tests/native/symcount_host.cpp) and run "as 256 lanes would" over whole blocks against a straightforward count over
(bitmaps, records, source): every length and every distance for the symbol functions; blocks of 0, 1, 7, 8, 9, 2047, 2048,
2049, 65535 and 65536 positions -- random parses, literals only, one symbol only, every symbol -- with a source of exactly
n bytes and the bitmaps' bits behind position n all set."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS = (0, 1, 7, 8, 9, 2047, 2048, 2049, 65535, 65536)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    exe = tmp_path_factory.mktemp("symcount") / "symcount_host"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "power-gzip_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "symcount_host.cpp"), "-o", str(exe)], check=True)

    def run(*args):
        r = subprocess.run([str(exe)] + [str(a) for a in args], capture_output=True, timeout=600)
        assert r.returncode == 0, (r.returncode, r.stdout.decode()[-2000:], r.stderr.decode()[-4000:])
        return r.stdout.decode().splitlines()
    return run


def test_every_length_and_every_distance_has_rfc1951_s_symbol(host):
    assert host("symbols") == ["symbols: 0 wrong"]


def test_the_gpu_test_s_cases_are_what_they_claim():
    """tests/symcount_cases.py: the block built for it uses every length and every distance symbol and every literal in the
    oracle's parse; the batch has every length, all-literal and one-symbol blocks, and every history"""
    import symcount_cases as S
    c = S.counts(S.every_symbol_block())
    assert (c[:256] > 0).all() and (c[257:286] > 0).all() and (c[286:316] > 0).all() and c[256] == 1
    batch = S.small_batch()
    assert 30 <= len(batch) <= 45 and len({name for name, _, _ in batch}) == len(batch)
    assert {len(d) for _, d, h in batch if h == 0} >= set(S.LENGTHS) and {h for _, _, h in batch} == set(S.HISTORIES) | {0}
    by = {name: S.counts(d, h) for name, d, h in batch}
    z = by["block/zeros"]                                        # one literal, then distance 1 all the way in the two longest length symbols
    assert z[:256].sum() == 1 and z[286] == z[284] + z[285] == z[257:286].sum() >= 254 and z[287:].sum() == 0
    assert by["block/random"][:256].sum() == 65536 and (by["block/random"][:256] > 0).all()
    assert by["block/ff"][255] == 1 and by["block/ff"][:255].sum() == 0
    assert (by["block/text33"][:256] > 0).sum() == 33


@pytest.mark.parametrize("seed", [1, 20])
def test_whole_blocks_as_256_lanes_would_count_them(host, seed):
    out = host("blocks", seed)
    assert len(out) == 5 * len(LENGTHS) and all(line.endswith(" 0 wrong") for line in out), out
    assert [int(line.split()[2]) for line in out[::5]] == list(LENGTHS)
    # the cases are what they are meant to be: no record where there is no room for a match, records in the large blocks
    assert all(" 0 records" in line for line in out[:10]) and all(" 0 records" not in line for line in out[-5:] if "kind 1" not in line)
