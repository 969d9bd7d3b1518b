"""The tiny `Coach` runs of the GPU tests: the toy image folder and the mode-0 configuration (resume, training record,
loss options), the synthetic DTU scene and the mode-2 configuration (held-out validation), and how the tests seed, train
and compare them.

pytest does not rewrite the asserts of a helper module: every assert here carries its message."""
import random
from pathlib import Path

import numpy as np
import torch
from PIL import Image

from helpers.engines import FIELDS, snapshot


def _finish(cfg):
    cfg.log.exp_dir = cfg.log.exp_dir / cfg.log.exp_name
    cfg.log.logging_dir = cfg.log.exp_dir / cfg.log.logging_dir
    return cfg


# ------------------------------------------------------------------------------------------------ mode 0 on toy images
def toys(root):
    root.mkdir(parents=True)
    rng = np.random.RandomState(0)
    for i in range(3):
        Image.fromarray(rng.randint(0, 255, (90, 120, 3), dtype=np.uint8)).save(root / f"{i}.png")


def mode0_cfg(toys_dir, out, *extra, max_steps=6):
    """the tiny mode-0 configuration of test_coach_mode0_trains_and_saves: validation off, cosine schedule with warm-up,
    nested dropout, accumulation 2, a checkpoint + trainer state every 3 steps"""
    from view_neti_amd.compat import config as C
    return _finish(C.parse(C.RunConfig, [
        "--data.train_data_dir", str(toys_dir), "--data.placeholder_object_token", "<toy>", "--data.resolution", "64",
        "--data.dataloader_num_workers", "0", "--data.augmentation_key", "5", "--model.word_embedding_dim", "128",
        "--model.arch_view_net", "15", "--model.arch_view_disable_tl", "False", "--model.arch_mlp_hidden_dims", "64",
        "--model.use_nested_dropout", "True", "--optim.max_train_steps", str(max_steps), "--optim.train_batch_size", "2",
        "--optim.gradient_accumulation_steps", "2", "--optim.mixed_precision", "fp16", "--optim.lr_scheduler", "cosine",
        "--optim.lr_warmup_steps", "2", "--log.save_steps", "3", "--log.save_trainer_state", "true",
        "--eval.validation_steps", "1000", "--log.exp_dir", str(out), "--log.exp_name", "run", *extra]))


def seed_all(s):
    torch.manual_seed(s)
    np.random.seed(s)
    random.seed(s)


def coach(cfg, seed=0):
    from view_neti_amd.compat.coach import Coach
    seed_all(seed)
    return Coach(cfg)


def train_counting(coach):
    """coach.train() -> number of optimizer steps it performed"""
    n, step = [0], coach.engine.step

    def counting():
        done = step()
        n[0] += bool(done)
        return done
    coach.engine.step = counting
    coach.train()
    coach.engine.step = step
    return n[0]


def end_state(coach):
    return snapshot(coach.engine, FIELDS)


def assert_end(want, got):
    for f in ("params", "exp_avg", "exp_avg_sq", "scaler", "rng_state", "seg_step", "opt_step"):
        assert torch.equal(want[f], got[f]), f"{f} differs from the uninterrupted run"
    assert want["hyper"][0] == got["hyper"][0], f"lr {got['hyper'][0]!r} differs from the uninterrupted run's {want['hyper'][0]!r}"


def mapper_tensors(path):
    ck = torch.load(path, map_location="cpu", weights_only=False)
    return {(k, name): t for k, e in ck["mappers"].items() for name, t in e["state_dict"].items()}


# ------------------------------------------------------------------------------------------------ mode 2 on a DTU scene
def dtu_scene(root: Path, scans, seed=1):
    cal = root / "data" / "dtu" / "Calibration" / "cal18"
    cal.mkdir(parents=True)
    rng = np.random.RandomState(seed)
    mats = rng.randn(49, 3, 4) * np.array([[1e3, 1e3, 1e3, 1e5]])
    for i in range(49):
        np.savetxt(cal / f"pos_{i + 1:03d}.txt", mats[i])
    from view_neti_amd.compat.dataset import TextualInversionDataset
    out = []
    for scan in scans:
        d = root / "data" / "dtu" / "Rectified" / scan
        d.mkdir(parents=True)
        for c in range(49):
            Image.fromarray(rng.randint(0, 255, (120, 160, 3), dtype=np.uint8)).save(
                d / TextualInversionDataset.dtu_cam_and_lighting_to_fname(c, "3"))
        out.append(d)
    return out


def mode2_cfg(scan, out, name, *extra):
    from view_neti_amd.compat import config as C
    return _finish(C.parse(C.RunConfig, [
        "--learnable_mode", "2", "--data.train_data_dir", str(scan), "--data.placeholder_object_token", "<object>",
        "--data.camera_representation", "dtu-12d", "--data.dtu_subset", "3", "--data.dtu_preprocess_key", "1",
        "--data.augmentation_key", "5", "--data.dataloader_num_workers", "0", "--model.word_embedding_dim", "128",
        "--model.arch_view_net", "15", "--model.arch_view_disable_tl", "False", "--model.arch_mlp_hidden_dims", "64",
        "--model.use_nested_dropout", "True", "--model.pe_sigma_exp_key", "2", "--optim.max_train_steps", "4",
        "--optim.train_batch_size", "3", "--optim.gradient_accumulation_steps", "1", "--optim.mixed_precision", "fp16",
        "--log.save_steps", "2", "--eval.validation_steps", "1000", "--eval.num_denoising_steps", "2",
        "--eval.num_validation_images", "1", "--eval.validation_seeds", "[0]", "--log.exp_dir", str(out),
        "--log.exp_name", name, *extra]))


def train_from_cfg(cfg):
    """seed as the command line does (torch from cfg.seed), build the Coach, train -> the Coach"""
    from view_neti_amd.compat.coach import Coach
    torch.manual_seed(cfg.seed)
    np.random.seed(0)
    random.seed(0)
    coach = Coach(cfg)
    coach.train()
    return coach
