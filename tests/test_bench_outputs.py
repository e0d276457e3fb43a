"""CPU: bench.py's command line and the writer behind --dump-outputs (float files, one seeded row sample past the size bound)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_plain_run_is_the_default_and_full_is_an_option():
    a = bench.parse_args(["--gpus", "1", "--steps", "5", "--warmup", "2"])
    assert a.steps == 5 and a.warmup == 2 and a.full is False and a.dump_outputs is None
    a = bench.parse_args(["--full", "--dump-outputs", "out"])
    assert a.full is True and a.dump_outputs == "out"


def test_outputs_are_written_as_float_arrays(tmp_path):
    rng = np.random.default_rng(1)
    x = rng.normal(size=(50, 3))
    names = bench.write_outputs(str(tmp_path), {"positions": x, "ids": np.arange(50, dtype=np.int32),
                                                "half": x.astype(np.float32)}, {"energy": -3.5})
    assert names == ["energy", "half", "ids", "positions"]
    assert sorted(os.listdir(tmp_path)) == ["energy.npy", "half.npy", "ids.npy", "positions.npy"]
    assert np.array_equal(np.load(tmp_path / "positions.npy"), x)
    ids = np.load(tmp_path / "ids.npy")
    assert ids.dtype == np.float64 and np.array_equal(ids, np.arange(50))
    assert np.load(tmp_path / "half.npy").dtype == np.float32
    e = np.load(tmp_path / "energy.npy")
    assert e.dtype == np.float64 and e.shape == (1,) and e[0] == -3.5


def test_large_outputs_keep_one_fixed_sample_of_rows(tmp_path):
    n = 10000
    x = np.arange(3 * n, dtype=np.float64).reshape(n, 3)
    f = -x
    limit = 100_000
    for d in ("a", "b"):
        bench.write_outputs(str(tmp_path / d), {"positions": x, "forces": f}, {"energy": 1.0}, limit=limit)
    total = sum(os.path.getsize(tmp_path / "a" / p) for p in os.listdir(tmp_path / "a"))
    assert total <= limit
    pa, fa = np.load(tmp_path / "a" / "positions.npy"), np.load(tmp_path / "a" / "forces.npy")
    assert 0 < len(pa) < n and len(pa) == len(fa)
    rows = pa[:, 0] / 3
    assert np.all(np.diff(rows) > 0) and np.array_equal(fa, -pa)                     # ascending rows, the same in every array
    assert np.array_equal(pa, np.load(tmp_path / "b" / "positions.npy"))              # the same rows on every run
    assert np.load(tmp_path / "a" / "energy.npy")[0] == 1.0
