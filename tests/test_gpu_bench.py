"""-m gpu: bench.py end to end on one GPU.  With --full (every leg but the CPU baseline), on the default workload and one GIN workload: the
JSON line must carry the contract's fields, the roofline object of the kernels the step really runs and a whole-step figure.  A plain run
(the headline alone) with --dump-outputs: the line, and what the last timed step computed, identical inputs from run to run."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("workload", ["c3", "c2"])
def test_bench_line_single_gpu(dev, workload):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--workload", workload, "--steps", "5", "--warmup", "2", "--full", "--no-cpu-baseline"]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=root)
    assert res.returncode == 0, res.stderr[-3000:]
    line = json.loads(res.stdout.strip().splitlines()[-1])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data",
                "config", "roofline", "cpu_baseline", "gemm_precision", "value_fp32_exact", "full_step"):
        assert key in line, key
    assert line["n_gpus"] == 1 and line["steps"] == 5 and line["value"] > 0 and line["vs_baseline"] is None and line["cpu_baseline"] is None
    roof = line["roofline"]
    assert roof["bound"] == "hbm" and 0 < roof["frac"] <= 1.2 and roof["timing"] == "in_step" and roof["backward"]["us_all_launches"] > 0
    assert line["full_step"]["ms_per_step"] > line["ms_per_step"]
    if workload == "c3":
        assert "one-launch" in line["gemm_precision"] and "x6" in line["gemm_precision"]          # the forward the step really took
    else:
        assert "staged" in line["gemm_precision"]


def test_bench_plain_run_dumps_outputs(dev, tmp_path):
    """The plain run times the hot path and nothing else; --dump-outputs writes what its last step computed, in float32 and within 64 MB, and
    two runs with the same arguments start from the same inputs, so they compute the same arrays (up to the order of float sums)."""
    import numpy as np
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    dumps = []
    for run in ("a", "b"):
        out = tmp_path / run
        cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--dump-outputs", str(out)]
        res = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=root)
        assert res.returncode == 0, res.stderr[-3000:]
        line = json.loads(res.stdout.strip().splitlines()[-1])
        assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0 and line["value"] > 0
        assert line["higher_is_better"] is True and line["dtype"] == "f32" and line["unit"] == "million edges/s"
        assert line["roofline"] is None and line["full_step"] is None and line["cpu_baseline"] is None and line["value_fp32_exact"] is None
        files = sorted(out.iterdir())
        assert sum(f.stat().st_size for f in files) <= 64 * 2**20
        manifest = line["dump_outputs"]["arrays"]
        assert sorted(f.name for f in files) == sorted(f"{k}.npy" for k in manifest)
        assert {"att", "att_log_logits", "out_l0", "out_l3", "grad_emb", "grad_x_l0", "grad_x_l3"} <= set(manifest)
        assert any(m["rows_kept"] is not None and m["rows_kept"] < m["shape"][0] for m in manifest.values())     # C3's outputs are sampled
        arrays = {f.stem: np.load(f) for f in files}
        for name, a in arrays.items():
            assert a.dtype == np.float32 and a.size > 0 and np.isfinite(a).all(), name
            assert a.shape[1:] == tuple(manifest[name]["shape"][1:]), name
        dumps.append(arrays)
    for name, a in dumps[0].items():
        b = dumps[1][name]
        assert a.shape == b.shape and np.allclose(a, b, rtol=1e-4, atol=1e-5 * max(1.0, float(np.abs(a).max()))), name
