"""bench.py with TWO ranks on the one visible GPU (VOXE_BENCH_BACKEND=gloo: the ranks share the device and exchange
through host staging): the N > 1 code path -- x-slab reduce-scatter / all-to-all / all-reduce of the workspace gradient
region, the sharded fused Adam, the all-gather of the packed grid, autotune -- runs with the real kernels and must leave
every rank with the same packed grid.  Not a measurement (gloo), a correctness run."""
import json
import os
import socket
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


@pytest.mark.timeout(600)
@pytest.mark.parametrize("exchange,expect", [("reduce-scatter", "reduce-scatter + sharded step"), ("all-to-all", "all-to-all + local sum"),
                                             ("all-reduce", "all-reduce + replicated step"),
                                             ("pipelined", "pipelined direct exchange"), ("auto", "")])
def test_two_rank_bench_on_one_gpu(exchange, expect):
    env = dict(os.environ, VOXE_BENCH_BACKEND="gloo", VOXE_GRAD_EXCHANGE=exchange, VOXE_BENCH_PRE_WARM_MS="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1",
           "--grid", "32", "--image", "96", "--samples", "64", "--full"]
    res = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=560)
    assert res.returncode == 0, res.stderr[-2000:]
    line = [l for l in res.stdout.strip().splitlines() if l.startswith("{")][-1]
    out = json.loads(line)
    assert out["n_gpus"] == 2 and out["scaling"] == "weak" and out["value"] > 0
    cfg = out["config"]
    assert cfg["replicas_consistent"] is True and cfg["backend"] == "gloo" and cfg["optimizer"] == "fused"
    assert cfg["grad_exchange"].startswith(expect)
    assert cfg["rays_per_gpu_per_step"] == 96 * 96
    assert cfg["per_rank"]["first_camera"] == [3, 40] and all(x > 0 for x in cfg["per_rank"]["bwd_ms"])
    assert cfg["views"]["count"] == 20 and cfg["views"]["cameras_of_rank0"][:3] == [3, 8, 13]      # the steps cycle through the view set
    if exchange == "auto":
        assert set(cfg["exchange_autotune_ms"]) == {"reduce-scatter", "all-to-all", "all-reduce", "pipelined"}


@pytest.mark.timeout(600)
def test_two_rank_strong_scaling_bench_on_one_gpu():
    """`--scaling strong`: ONE camera split into row bands (what a multi-GPU SDS iteration does), same exchange; the job's
    rays per step are the image's, not N images'"""
    env = dict(os.environ, VOXE_BENCH_BACKEND="gloo", VOXE_GRAD_EXCHANGE="reduce-scatter", VOXE_BENCH_PRE_WARM_MS="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1",
           "--grid", "32", "--image", "100", "--samples", "64", "--scaling", "strong", "--full"]
    res = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=560)
    assert res.returncode == 0, res.stderr[-2000:]
    out = json.loads([l for l in res.stdout.strip().splitlines() if l.startswith("{")][-1])
    assert out["n_gpus"] == 2 and out["scaling"] == "strong" and out["value"] > 0
    cfg = out["config"]
    assert cfg["replicas_consistent"] is True and cfg["rows_of_rank0"] == [0, 48]     # 13 tile rows of 8 pixels: 6 + 7
    assert cfg["rays_per_gpu_per_step"] == 48 * 100
    # value counts the IMAGE once per step
    assert abs(out["value"] - 100 * 100 * out["steps"] / (out["ms_per_step"] * 1e-3 * out["steps"])) < 1e-3 * out["value"]


@pytest.mark.timeout(600)
@pytest.mark.parametrize("exchange", ["reduce-scatter", "all-to-all", "all-reduce", "pipelined"])
def test_two_ranks_equal_one_process(exchange):
    """4 optimiser steps of the 2-rank job (one camera per rank, gradient exchange, sharded / replicated fused Adam) land
    on the parameters of ONE process that accumulates both cameras' gradients before each step -- up to the float
    rounding of the gradient sums (atomics inside a launch, and a + b across ranks vs accumulation in one buffer)"""
    env = dict(os.environ)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(ROOT, "tests", "two_rank_worker.py"), exchange]
    res = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=560)
    assert res.returncode == 0, res.stderr[-2000:]
    line = [l for l in res.stdout.strip().splitlines() if l.startswith("{")][-1]
    ranks = json.loads(line)["ranks"]
    assert len(ranks) == 2
    for r in ranks:
        assert r["mode"].startswith(exchange if exchange != "all-reduce" else "all-reduce")
        assert r["moved"] > 1e-3                                   # the run really trained
        # Adam's first steps turn the rounding noise of near-zero gradients into +-lr moves: measure against the movement
        # (observed: features 3e-7, densities 3e-4 for a movement of 5e-2)
        assert r["rel_densities"] < 0.05 * r["moved"] and r["rel_features"] < 0.05 * r["moved"], r


@pytest.mark.timeout(600)
def test_two_rank_sds_loop_equals_one_process():
    """the ray-sharded SDS edit loop (row bands per rank, all-gathered image, replicated guidance, one gradient
    all-reduce) with 2 ranks vs the same 12 iterations in one process"""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(ROOT, "tests", "two_rank_sds_worker.py")]
    res = subprocess.run(cmd, cwd=ROOT, env=dict(os.environ), capture_output=True, text=True, timeout=560)
    assert res.returncode == 0, res.stderr[-2500:]
    line = [l for l in res.stdout.strip().splitlines() if l.startswith("{")][-1]
    for r in json.loads(line)["ranks"]:
        assert r["moved"] > 1e-3
        assert r["rel_densities"] < 0.05 * r["moved"] and r["rel_features"] < 0.05 * r["moved"], r


@pytest.mark.timeout(600)
def test_default_bench_line_has_the_contract_fields():
    """the driver's N = 1 command line (short): one JSON line with the contract's fields, the roofline object fed by a PMC
    summary that belongs to these kernel sources (not stale), the CPU / same-GPU baselines; r06: the steps cycle through 20 cameras
    of the 100-view set (value = mean over views) and `roofline.frac` is the utilisation of the ceiling that binds (<= 1)"""
    env = dict(os.environ, VOXE_BENCH_PRE_WARM_MS="20")
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "4", "--warmup", "2", "--cpu-sample", "40", "--full"],
                         cwd=ROOT, env=env, capture_output=True, text=True, timeout=560)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [l for l in res.stdout.strip().splitlines() if l.startswith("{")]
    assert len(lines) == 1
    out = json.loads(lines[0])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
                "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert key in out, key
    assert out["n_gpus"] == 1 and out["steps"] == 4 and out["dtype"] == "f32" and out["value"] > 1e7
    roof = out["roofline"]
    assert roof["alg"]["frac_of_hbm_peak"] > 0 and roof["alg"]["bytes_per_launch"] > 0          # SURVEY 8(d)'s requested-bytes figure
    if roof["physical"].get("stale"):
        # the committed PMC summary was collected on other kernel sources (a kernel edit since the last tools/gpu_pmc.sh run):
        # the line must say so instead of mixing those counters with this run's timings -- and states NO fraction
        assert "source_hash" in roof["physical"]["reason"] and roof["traffic"] is None and roof["frac"] is None
    else:
        assert roof["traffic"] > 0 and roof["bound"] == roof["physical"]["binding"]
        assert roof["physical"]["binding"] in ("lds_issue", "valu_issue", "hbm") and 0 < roof["physical"]["binding_frac"] <= 1
        assert 0 < roof["frac"] <= 1 and abs(roof["frac"] - roof["achieved"] / roof["peak"]) < 1e-3
        assert abs(roof["frac"] - roof["physical"]["binding_frac"]) < 1e-3
        assert roof["physical_other"]["kernel"].startswith("voxe::render_fwd_tile")   # tile4 (lean, r05) or tile (general)
    assert out["ms_per_step_min"] <= out["ms_per_step_median"] <= out["ms_per_step_max"] and out["config"]["untimed_warmup_ms"] >= 5
    assert out["cpu_baseline"]["reps"] == 3 and out["gpu_baseline"]["reps"] == 3
    assert out["cpu_baseline"]["kind"] == "port" and out["cpu_baseline"]["value"] > 0
    assert out["gpu_baseline"]["value"] > 0 and out["gpu_baseline"]["speedup"] > 10
    views = out["config"]["views"]
    assert views["count"] == 20 and len(views["cameras_of_rank0"]) == 20 and views["cameras_of_rank0"][:4] == [3, 8, 13, 18]
    assert views["ms_per_step_by_view"][:4] == [x for x in views["ms_per_step_by_view"][:4] if x and x > 0]     # steps 0..3 rendered views 0..3
    assert views["min_rays_per_s"] <= views["max_rays_per_s"] and views["min_rays_per_s"] > 1e7
