"""`optim.mixed_precision: bf16` (training/coach.py:796-802): the same kernels built with -DVN_BF16 (libvneti_hip_bf16.so:
bf16 storage and MFMA operands, f32 accumulation and statistics, no loss scaling).  A process computes in ONE 16-bit
format, so every case runs in a child process with VNETI_PRECISION=bf16 (tests/helpers/bf16_step_check.py) and is checked
against the CPU oracle on bf16-rounded weights.

Bars: bf16 keeps 8 significant bits where fp16 keeps 11, so one rounding is 8x coarser (2^-9 = 2e-3 relative) and the
north star's 1e-3 (stated for fp16) becomes 8e-3 on the loss; the mapper gradient has to point the same way (cosine
>= 0.995) — a transposed operand, a wrong MFMA opcode or f16 bits read as bf16 give O(1) errors.  What these bars cannot
see, a kernel that is subtly wrong in bf16 only, is tests/test_kernels_bf16_gpu.py's job: per-kernel parity of the bf16 library."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(*args, timeout=1500):
    env = dict(os.environ, VNETI_PRECISION="bf16")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "helpers", "bf16_step_check.py"), *map(str, args)],
                       capture_output=True, text=True, timeout=timeout, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    for line in reversed(r.stdout.strip().splitlines()):
        if line.startswith("{"):
            return json.loads(line)
    raise AssertionError("no JSON line:\n" + r.stdout[-2000:])


@pytest.mark.timeout(900)
@pytest.mark.parametrize("name", ["tiny", "tiny21"])
def test_bf16_train_step_tiny_matches_oracle(name):
    res = _run(name, 2, 64, 64)
    print("[bf16]", res)
    assert res["finite"] and res["opt_step"] == 1
    assert res["loss_rel"] < 8e-3 and res["grad_cos"] > 0.995 and res["grad_rel"] < 0.15
    assert res["adamw_dev_over_lr"] < 0.05


@pytest.mark.timeout(2400)
def test_bf16_full_size_matches_oracle():
    """BASELINE config 2's shapes (SD-1.5, 512^2) at bs 1 in bf16 against the fp32 oracle on bf16-rounded weights"""
    res = _run("sd15", 1, 512, 512, timeout=2300)
    print("[bf16 full size]", res)
    assert res["finite"] and res["loss_rel"] < 8e-3 and res["grad_cos"] > 0.995 and res["latents_rel"] < 8e-3


@pytest.mark.timeout(900)
def test_bf16_coach_trains_and_saves(tmp_path):
    """the reference's own CLI surface with --optim.mixed_precision bf16: Coach selects the bf16 library, trains, saves"""
    import numpy as np
    from PIL import Image
    root = tmp_path / "toys"
    root.mkdir()
    rng = np.random.RandomState(0)
    for i in range(3):
        Image.fromarray(rng.randint(0, 255, (90, 120, 3), dtype=np.uint8)).save(root / f"{i}.png")
    code = f"""
import sys, torch
sys.path.insert(0, {ROOT!r})
from view_neti_amd import lib
from view_neti_amd.compat import config as C
from view_neti_amd.compat.coach import Coach
cfg = C.parse(C.RunConfig, ["--data.train_data_dir", {str(root)!r}, "--data.placeholder_object_token", "<toy>",
    "--data.resolution", "64", "--data.dataloader_num_workers", "0", "--model.word_embedding_dim", "128",
    "--model.arch_view_net", "15", "--model.arch_view_disable_tl", "False", "--model.arch_mlp_hidden_dims", "64",
    "--optim.max_train_steps", "3", "--optim.train_batch_size", "2", "--optim.gradient_accumulation_steps", "1",
    "--optim.mixed_precision", "bf16", "--log.save_steps", "100", "--eval.validation_steps", "100",
    "--log.exp_dir", {str(tmp_path / "out")!r}, "--log.exp_name", "bf16"])
cfg.log.exp_dir = cfg.log.exp_dir / cfg.log.exp_name
cfg.log.logging_dir = cfg.log.exp_dir / cfg.log.logging_dir
torch.manual_seed(cfg.seed)
coach = Coach(cfg)
assert lib.precision() == "bf16" and coach.engine.unet.pred.dtype == torch.bfloat16
p0 = coach.engine.params.clone()
coach.train()
e = coach.engine
assert e.opt_step.item() == 3 and torch.isfinite(e.params).all() and not torch.equal(p0, e.params)
assert float(e.scaler[0]) == 1.0
print("BF16_COACH_OK")
"""
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=800)
    assert r.returncode == 0 and "BF16_COACH_OK" in r.stdout, r.stderr[-3000:]
    assert (tmp_path / "out" / "bf16" / "mapper-final_object.pt").exists()
