"""nxz_batch_shuffle and nxz_batch_unshuffle (include/nxz_engine.h) are part of what libnxz_engine.so exports: named in the version
script and present in the built library's dynamic symbol table, beside the tile query the tests read."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["nxz_batch_shuffle", "nxz_batch_unshuffle", "nxz_shuffle_tile_elems"]


@pytest.mark.parametrize("name", NAMES)
def test_named_in_the_version_script(name):
    text = open(os.path.join(ROOT, "power-gzip_amd", "csrc", "nxz_engine.map")).read()
    head = text[:text.index("local:")]
    assert re.search(r"\b%s;" % name, head), name


@pytest.mark.parametrize("name", NAMES)
def test_exported_by_the_built_library(name):
    lib = os.path.join(ROOT, "power-gzip_amd", "libnxz_engine.so")
    assert os.path.exists(lib), "build() has not run"
    out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    assert re.search(r" T %s(@@NXZ_ENGINE_1)?$" % name, out, re.M), name


def test_declared_in_the_public_header():
    text = open(os.path.join(ROOT, "include", "nxz_engine.h")).read()
    assert "#define NXZ_SHUFFLE_ELEM_MAX 256" in text
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, text), name
