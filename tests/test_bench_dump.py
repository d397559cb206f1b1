"""not gpu: bench.dump_outputs (--dump-outputs) writes one .npy file per array, within the byte budget, in float32 (float64 stays
float64), and samples the same rows of an array of the same shape on every run."""
import numpy as np
import torch

import bench


def _arrays():
    g = torch.Generator().manual_seed(0)
    return {"big": torch.randn(20000, 64, generator=g), "wide": torch.randn(5000, 256, generator=g),
            "small": torch.randn(100, 8, generator=g), "vec64": torch.randn(1000, generator=g, dtype=torch.float64),
            "half": torch.randn(300, 16, generator=g).to(torch.bfloat16)}


def test_dump_outputs_under_budget_writes_everything_whole(tmp_path):
    arrays = _arrays()
    manifest = bench.dump_outputs(arrays, str(tmp_path))
    assert set(manifest) == set(arrays) and sorted(f.name for f in tmp_path.iterdir()) == sorted(f"{k}.npy" for k in arrays)
    for name, t in arrays.items():
        a = np.load(tmp_path / f"{name}.npy")
        assert a.dtype == (np.float64 if name == "vec64" else np.float32), name
        assert np.array_equal(a, t.double().numpy() if name == "vec64" else t.float().numpy()), name
        assert manifest[name]["shape"] == list(t.shape) and manifest[name]["rows_kept"] is None


def test_dump_outputs_samples_large_arrays_into_the_budget(tmp_path):
    arrays, budget = _arrays(), 2_000_000
    manifest = [bench.dump_outputs(arrays, str(tmp_path / run), budget=budget) for run in ("a", "b")][0]
    data = sum(np.load(f).nbytes for f in (tmp_path / "a").glob("*.npy"))
    assert data <= budget
    for name, t in arrays.items():
        a, b = np.load(tmp_path / "a" / f"{name}.npy"), np.load(tmp_path / "b" / f"{name}.npy")
        assert np.array_equal(a, b), name                                  # the same rows in every run
        if name in ("big", "wide"):                                        # above the whole-array limit: sampled
            assert manifest[name]["rows_kept"] == a.shape[0] < t.shape[0] and manifest[name]["shape"] == list(t.shape)
            where = {r.tobytes(): i for i, r in enumerate(t.numpy())}
            idx = [where[r.tobytes()] for r in a]                          # every kept row is a row of the array, in order
            assert all(i < j for i, j in zip(idx, idx[1:])), name
        else:
            assert manifest[name]["rows_kept"] is None and a.shape == tuple(t.shape), name
