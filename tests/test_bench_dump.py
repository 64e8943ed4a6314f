"""CPU: bench.py's --dump-outputs writer (what the last timed step computed, as .npy, under the size limit) and the
argument checks around it.  The GPU run of the option is tests/test_bench_gpu.py."""
import os

import numpy as np
import pytest
import torch

import bench


def test_small_output_is_written_whole(tmp_path):
    x = torch.arange(1024 * 7, dtype=torch.float32).reshape(1024, 7)
    info = bench.dump_outputs(str(tmp_path), {"logits": x}, 0, 1)
    assert info == {"logits": {"shape": [1024, 7]}}
    got = np.load(tmp_path / "logits.npy")
    assert got.dtype == np.float32 and np.array_equal(got, x.numpy())
    assert sorted(os.listdir(tmp_path)) == ["logits.npy"]


def test_large_output_is_a_seeded_sample_of_rows(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 200_000)
    x = torch.randn(64, 20, 30, generator=torch.Generator().manual_seed(0))  # 153,600 bytes over two ranks' budget
    runs = []
    for d in ("a", "b"):
        info = bench.dump_outputs(str(tmp_path / d), {"featuregram": x}, 1, 2)
        k = info["featuregram_rank1"]["sampled_rows"]
        rows = np.load(tmp_path / d / "featuregram_rows_rank1.npy")
        got = np.load(tmp_path / d / "featuregram_rank1.npy")
        assert rows.dtype == np.float64 and got.dtype == np.float32 and got.shape == (k, 20, 30) and len(rows) == k
        assert np.all(np.diff(rows) > 0) and np.array_equal(got, x.numpy()[rows.astype(np.int64)])
        assert sum(f.stat().st_size for f in (tmp_path / d).iterdir()) <= bench.DUMP_LIMIT_BYTES // 2
        runs.append((rows, got))
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])


def test_arguments():
    a = bench.parse_args(["--steps", "3", "--dump-outputs", "out"])
    assert a.steps == 3 and a.dump_outputs == "out"
    assert bench.parse_args([]).dump_outputs is None
    for argv in (["--steps", "0"], ["--dry-run", "--dump-outputs", "out"]):
        with pytest.raises(SystemExit):
            bench.parse_args(argv)
