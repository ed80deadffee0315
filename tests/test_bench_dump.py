"""CPU test of bench.py --dump-outputs: the same seeded sample every run, output bytes past the job's byte count zeroed,
float32 / float64 only, never more than the limit."""
import importlib
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("power-gzip_amd")


def _fake_batch(n, seed=3):
    g = np.random.default_rng(seed)
    dst = torch.from_numpy(g.integers(0, 256, (n, 4096), dtype=np.uint8))
    res = np.zeros(n, pkg.RESULT_DTYPE)
    for f in pkg.RESULT_DTYPE.names:
        res[f] = g.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    res["tpbc"] = g.integers(0, 4097, n)
    return dst, res


def test_dump_of_a_deflate_batch(tmp_path):
    import bench
    n = 1000
    dst, res = _fake_batch(n)
    out = bench.dump_deflate(torch, dst, res, n)
    idx = out["sample_index"].astype(np.int64)
    assert len(idx) == bench.DUMP_ROWS and (np.diff(idx) > 0).all() and (idx == bench.dump_sample(n)).all()
    for k, i in enumerate(idx):
        t = int(res["tpbc"][i])
        assert (out["compressed"][k, :t] == dst[i, :t].numpy()).all() and not out["compressed"][k, t:].any()
    assert out["results"].shape == (n, len(pkg.RESULT_DTYPE.names))
    assert (out["results"][:, pkg.RESULT_DTYPE.names.index("crc")] == res["crc"]).all()      # float64 holds every u32 exactly
    bench.write_dump(str(tmp_path / "d"), out)
    for name, a in out.items():
        back = np.load(tmp_path / "d" / (name + ".npy"))
        assert back.dtype in (np.float32, np.float64) and (back == a).all()


def test_dump_stays_under_the_limit():
    import bench
    n = 10000
    res = np.zeros(n, pkg.RESULT_DTYPE)
    idx = bench.dump_sample(n)
    assert list(bench.dump_results(res, idx, n * 64)) == ["results"]
    got = bench.dump_results(res, idx, n * 64 - 1)                 # every job's records do not fit: the sampled jobs' only
    assert list(got) == ["results_sample"] and got["results_sample"].shape == (len(idx), len(pkg.RESULT_DTYPE.names))
    assert bench.dump_sample(n).tolist() == idx.tolist()


def test_write_dump_refuses_more_than_the_limit(tmp_path):
    import bench
    with pytest.raises(SystemExit):
        bench.write_dump(str(tmp_path / "d"), {"x": np.zeros(bench.DUMP_LIMIT // 8 + 1, np.float64)})
    assert not (tmp_path / "d").exists()                           # refused before anything is written


def test_the_sampled_dump_always_fits():
    """when every job's records do not fit, the sample's do: the rows of the deflate configs (target stride) and of c5
    (inflated 64 KiB blocks) with their indices and records stay under the limit at any job count"""
    import bench
    per_record = 8 * len(pkg.RESULT_DTYPE.names)
    for row_bytes in (bench.STRIDE_OUT * 4, bench.BLOCK * 4):
        assert bench.DUMP_ROWS * (row_bytes + 8 + per_record) <= bench.DUMP_LIMIT
