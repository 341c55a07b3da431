"""bench.py's plain run and `--dump-outputs DIR`: what the last timed step computed, written so that two runs (or two builds)
can be compared array by array."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_samples_large_arrays_with_fixed_rows(tmp_path, monkeypatch):
    """arrays of at most DUMP_MAX_ROWS rows are written whole; larger ones as the same sorted, seeded rows in every call and
    for every array of that row count; float32 throughout; the 64 MB budget is enforced; a non-finite value writes nothing"""
    import bench

    monkeypatch.setattr(bench, "DUMP_MAX_ROWS", 1000)
    n = 5000
    rows = torch.arange(n, dtype=torch.float64)
    arrays = {"small": torch.ones(10, 1), "a": rows.view(n, 1, 1).expand(n, 2, 2), "b": rows.view(n, 1) * 2.0}
    written = bench.dump_outputs(str(tmp_path / "one"), arrays)
    bench.dump_outputs(str(tmp_path / "two"), arrays)
    assert written == {"small": 10, "a": 1000, "b": 1000}
    a, b = np.load(tmp_path / "one" / "a.npy"), np.load(tmp_path / "one" / "b.npy")
    assert a.dtype == np.float32 and a.shape == (1000, 4) and np.load(tmp_path / "one" / "small.npy").shape == (10, 1)
    picked = a[:, 0]
    assert np.all(np.diff(picked) > 0) and picked[-1] < n               # sorted rows, drawn without repetition
    assert np.array_equal(b[:, 0], 2.0 * picked)                          # the same rows for every array of that length
    for name in ("small", "a", "b"):
        assert np.array_equal(np.load(tmp_path / "one" / f"{name}.npy"), np.load(tmp_path / "two" / f"{name}.npy"))
    with pytest.raises(SystemExit, match="not finite"):
        bench.dump_outputs(str(tmp_path / "nan"), {"small": torch.ones(10, 1), "b": torch.tensor([[1.0], [float("nan")]])})
    assert not (tmp_path / "nan").exists()
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 1000)
    with pytest.raises(SystemExit):
        bench.dump_outputs(str(tmp_path / "three"), arrays)


def _bench(args, pre_warm_ms):
    env = dict(os.environ, VOXE_BENCH_PRE_WARM_MS=str(pre_warm_ms))
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], cwd=ROOT, env=env, capture_output=True, text=True,
                         timeout=560)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [l for l in res.stdout.strip().splitlines() if l.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_plain_bench_line_and_outputs_do_not_depend_on_the_pre_warm(tmp_path):
    """a plain run prints the headline only; its outputs equal those of a --full run whose time-based clock-settling run took
    a different number of steps (the state of the timed steps depends on the arguments only) up to the rounding of the
    backward's atomics.  The last step renders camera 18, some of whose rays miss the grid: their disparity (NaN, like the
    reference's) is written as 0"""
    small = ["--grid", "32", "--image", "96", "--samples", "64", "--steps", "4", "--warmup", "1"]
    plain = _bench(small + ["--dump-outputs", str(tmp_path / "plain")], 20)
    full = _bench(small + ["--dump-outputs", str(tmp_path / "full"), "--full", "--no-cpu-baseline", "--no-gpu-baseline"], 80)
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "config"):
        assert key in plain, key
    assert not {"roofline", "secondary", "cpu_baseline", "gpu_baseline"} & set(plain)
    assert "roofline" in full and full["metric"] == plain["metric"] and full["unit"] == plain["unit"]
    assert plain["steps"] == 4 and plain["dtype"] == "f32" and plain["higher_is_better"] is True
    # value = rays of the job per step / wall-clock milliseconds per step (the latter rounded to 0.1 us in the line)
    assert abs(plain["value"] - 96 * 96 / (plain["ms_per_step"] * 1e-3)) < 1e-2 * plain["value"]
    assert plain["outputs"] == {"colour": 96 * 96, "depth": 96 * 96, "acc": 96 * 96, "disp": 96 * 96,
                                "densities": 32 ** 3, "features": 32 ** 3}
    for name, width in (("colour", 3), ("depth", 1), ("acc", 1), ("disp", 1), ("densities", 1), ("features", 3)):
        a, b = np.load(tmp_path / "plain" / f"{name}.npy"), np.load(tmp_path / "full" / f"{name}.npy")
        assert a.dtype == np.float32 and a.shape == b.shape and a.shape[1] == width and np.isfinite(a).all()
        # (Adam turns the rounding noise of near-zero gradients into +-lr moves: 5 steps at lr 1e-4)
        np.testing.assert_allclose(a, b, atol=2e-3, rtol=1e-3, err_msg=name)
    acc, disp = np.load(tmp_path / "plain" / "acc.npy"), np.load(tmp_path / "plain" / "disp.npy")
    missed = acc[:, 0] == 0
    assert missed.any() and (disp[missed] == 0).all() and (disp[~missed] > 0).all()
    from voxe_hip.workload import random_grid

    init = random_grid(32)[0].reshape(-1, 1).numpy()
    moved = np.abs(np.load(tmp_path / "plain" / "densities.npy") - init).max()
    assert 0 < moved < 2e-3                     # 5 Adam steps at lr 1e-4 since the initial grid, not the clock-settling run's
