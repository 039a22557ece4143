"""CPU: bench.py --dump-outputs writes the same float32 row sample on every run and stays inside
its byte budget."""
import numpy as np
import torch

import bench


def test_dump_outputs_sample_is_fixed_and_bounded(tmp_path, monkeypatch):
    n = 1000
    ct = (torch.arange(n * 40, dtype=torch.int64) % 251).to(torch.uint8).reshape(n, 40)
    st = torch.arange(n, dtype=torch.int32)
    monkeypatch.setattr(bench, "DUMP_BUDGET", 64 * 1024)
    for d in ("a", "b"):
        bench.dump_outputs(tmp_path / d, {"ct": ct, "status": st})
    rows = np.load(tmp_path / "a" / "rows.npy")
    assert rows.dtype == np.float64 and 1 < rows.size < n
    assert np.all(np.diff(rows) > 0) and rows[-1] < n
    total = 0
    for name in ("rows", "ct", "status"):
        a, b = np.load(tmp_path / "a" / f"{name}.npy"), np.load(tmp_path / "b" / f"{name}.npy")
        assert a.dtype in (np.float32, np.float64) and np.array_equal(a, b)
        total += a.nbytes
    assert total <= 64 * 1024
    idx = rows.astype(np.int64)
    assert np.array_equal(np.load(tmp_path / "a" / "ct.npy"), ct.numpy()[idx].astype(np.float32))
    assert np.array_equal(np.load(tmp_path / "a" / "status.npy")[:, 0], rows.astype(np.float32))


def test_dump_outputs_keeps_everything_that_fits(tmp_path):
    ss = torch.arange(64 * 32, dtype=torch.int64).remainder(256).to(torch.uint8).reshape(64, 32)
    bench.dump_outputs(tmp_path, {"ss": ss})
    assert np.array_equal(np.load(tmp_path / "rows.npy"), np.arange(64, dtype=np.float64))
    assert np.array_equal(np.load(tmp_path / "ss.npy"), ss.numpy().astype(np.float32))
