"""bench.py's contract (one JSON line; N ranks launched by torch.distributed.run) exercised on ONE GPU: the N > 1 control
flow — rendezvous on 127.0.0.1, per-rank engine, captured graph A / all-reduce / graph B, barrier + max-over-ranks timing,
rank 0 prints — runs with the gloo backend standing in for RCCL (VNETI_DIST_BACKEND=gloo; every rank uses cuda:0)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(cmd, env_extra):
    env = dict(os.environ, **env_extra)
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.strip().splitlines() if l.startswith("{")]
    assert len(lines) == 1, f"exactly ONE JSON line expected, got {len(lines)}: {r.stdout[-500:]}"
    return json.loads(lines[0])


def _same_outputs(a, b):
    """two runs' dumps: every array bit for bit, except the loss, whose per-block partial sums are added atomically in
    whatever order the blocks finish (csrc/elementwise.hip mse_loss_grad_kernel) and so may differ in the last bits"""
    import numpy as np
    for f in a:
        if f.startswith("loss"):
            assert np.allclose(a[f], b[f], rtol=1e-6, atol=0), f"loss differs between two runs: {a[f]} vs {b[f]}"
        else:
            assert np.array_equal(a[f], b[f]), f"{f} differs between two runs with the same arguments"


@pytest.mark.timeout(1200)
def test_bench_single_gpu_line_tiny():
    d = _run([sys.executable, "bench.py", "--model", "tiny", "--resolution", "64", "--batch", "2", "--steps", "3",
              "--warmup", "1", "--full", "--no-cpu-baseline"], {})
    assert d["n_gpus"] == 1 and d["steps"] == 3 and d["warmup"] == 1 and d["value"] > 0 and d["unit"] == "steps/s"
    assert d["higher_is_better"] is True and d["scaling"] == "weak" and d["dtype"] == "f16" and d["vs_baseline"] is None
    r = d["roofline"]
    assert r["bound"] == "mfma" and r["peak"] == 2500.0 and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-9
    assert r["algorithmic_bytes_per_launch"] > 0 and r["avg_launch_us"] > 0
    assert abs(d["ms_per_step"] * d["value"] - 1000.0) < 1.0


@pytest.mark.timeout(1200)
def test_bench_plain_run_is_lean_and_dumps_its_outputs(tmp_path):
    """a plain run prints the headline line and nothing measured beside it (no roofline, CPU leg or extras: those are
    --full); --dump-outputs writes what the last timed step computed, and two runs with the same arguments (on the same
    autotuner picks) compute the same bits"""
    import numpy as np
    cmd = [sys.executable, "bench.py", "--model", "tiny", "--resolution", "64", "--batch", "2", "--steps", "4", "--warmup", "2"]
    env = {"VNETI_AUTOTUNE_CACHE": str(tmp_path / "picks.json")}
    runs = []
    for name in ("a", "b"):
        d = _run(cmd + ["--dump-outputs", str(tmp_path / name)], env)
        assert d["n_gpus"] == 1 and d["steps"] == 4 and d["warmup"] == 2 and d["value"] > 0 and d["unit"] == "steps/s"
        assert d["higher_is_better"] is True and d["dtype"] == "f16" and d["metric"].startswith("TI train steps/sec")
        assert abs(d["ms_per_step"] * d["value"] - 1000.0) < 1.0
        assert "roofline" not in d and "cpu_baseline" not in d and "coach_steps_per_s" not in d["config"]
        out = {f[:-4]: np.load(tmp_path / name / f) for f in sorted(os.listdir(tmp_path / name))}
        assert sorted(out) == ["loss", "mapper_grads", "mapper_params", "unet_pred"]
        assert out["loss"].dtype == np.float64 and float(out["loss"][0]) == d["config"]["final_loss"]
        assert out["unet_pred"].shape == (2, 8, 8, 4)
        runs.append(out)
    a, b = runs
    for f in a:
        assert a[f].dtype in (np.float32, np.float64)
        assert f == "mapper_grads" or np.isfinite(a[f]).all()  # (an fp16 overflow step leaves its gradients non-finite)
    _same_outputs(a, b)


@pytest.mark.timeout(1200)
def test_bench_headline_runs_compute_the_same_bits(tmp_path):
    """the headline workload replays the committed tile picks (bench_picks.json): two plain runs with the same arguments
    and no picks file of their own compute the same bits"""
    import numpy as np
    env = {k: v for k, v in os.environ.items() if k != "VNETI_AUTOTUNE_CACHE"}
    runs = []
    for name in ("a", "b"):
        r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1", "--dump-outputs",
                            str(tmp_path / name)], cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-2000:]
        runs.append({f: np.load(tmp_path / name / f) for f in sorted(os.listdir(tmp_path / name))})
    a, b = runs
    assert sorted(a) == ["loss.npy", "mapper_grads.npy", "mapper_params.npy", "unet_pred.npy"]
    _same_outputs(a, b)


@pytest.mark.timeout(1200)
def test_bench_two_ranks_on_one_gpu():
    port = 29700 + os.getpid() % 200
    d = _run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
              "127.0.0.1", "--master-port", str(port), "bench.py", "--gpus", "2", "--model", "tiny", "--resolution", "64",
              "--batch", "2", "--steps", "3", "--warmup", "1", "--full"],
             {"VNETI_DIST_BACKEND": "gloo", "HSA_ENABLE_IPC_MODE_LEGACY": "0"})
    assert d["n_gpus"] == 2 and d["config"]["parallelism"] == "dp2" and d["config"]["global_batch"] == 4
    assert d["value"] > 0 and abs(d["ms_per_step"] * d["value"] - 2000.0) < 2.0  # whole-job rate: 2 ranks' steps / max time
    assert "cpu_baseline" not in d  # rank 0 at N = 1 only


@pytest.mark.timeout(1800)
def test_bench_eight_ranks_on_one_gpu():
    """the driver's SCALE run by construction (no 8-GPU node was ever available to the build): `bench.py --gpus 8` as eight
    ranks (gloo, sharing cuda:0) — weak scaling: global batch 8 x per-GPU batch, value = 8 ranks' steps / MAX rank time,
    every rank on rank 0's tile picks, per-rank timings populated, the exchange route named."""
    port = 29900 + os.getpid() % 90
    d = _run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "8", "--master-addr",
              "127.0.0.1", "--master-port", str(port), "bench.py", "--gpus", "8", "--model", "tiny", "--resolution", "64",
              "--batch", "2", "--steps", "3", "--warmup", "1", "--full"],
             {"VNETI_DIST_BACKEND": "gloo", "HSA_ENABLE_IPC_MODE_LEGACY": "0", "OMP_NUM_THREADS": "2"})
    c = d["config"]
    assert d["n_gpus"] == 8 and c["parallelism"] == "dp8" and c["global_batch"] == 16 and c["rccl_ranks"] == 8
    assert d["scaling"] == "weak" and abs(d["ms_per_step"] * d["value"] - 8000.0) < 8.0
    assert c["picks_identical_on_all_ranks"] is True
    assert 0 < c["rank_ms_per_step_min"] <= c["rank_ms_per_step_max"] and abs(c["rank_ms_per_step_max"] - d["ms_per_step"]) < 1e-6
    assert c["exchange_in_graph"] is False and "gloo" in c["exchange"]  # the one-graph route needs the nccl backend
    assert "cpu_baseline" not in d


@pytest.mark.timeout(1200)
def test_bench_self_launches_two_ranks():
    """the driver's own invocation: plain `python bench.py --gpus 2` (no launcher) must spawn the 2 ranks itself."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(VNETI_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "2", "--model", "tiny", "--resolution", "64", "--batch", "2",
                        "--steps", "3", "--warmup", "1"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.strip().splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["config"]["rccl_ranks"] == 2 and d["config"]["dist_backend"] == "gloo"
    assert d["config"]["rank0_ms_per_step"] <= d["ms_per_step"] * 1.0001
