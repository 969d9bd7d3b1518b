"""The reference's scripts/summarize_dtu.py (`compute_metrics`, `process_dtu_checkpoints`): LPIPS, SSIM and PSNR per seed
of the DTU novel-view results that scripts/inference.py wrote, averaged over the runs of each (dtu_subset, iteration).

The reference hard-codes its result globs, needs pandas and ends in `ipdb.set_trace()`; here the runs and iterations are
arguments and the CSV (the reference's columns) is written with the `csv` module.  `lpips_fn` may be injected (any
`lpips.LPIPS`-like callable); one with a `compare(preds [S, V, ...], gt [V, ...])` method (compat/lpips.py) computes the
ground truth's features once per run instead of once per seed.
"""
from __future__ import annotations

import csv
import glob
from pathlib import Path
from typing import Dict, List, Sequence, Tuple

import numpy as np
import torch

from .dtu_metrics import lpips_fn_batch, mse_to_psnr, ssim_fn_batch

COLUMNS = ("num_imgs", "dtu_subset", "iteration", "seed", "lpips", "ssim", "psnr")


def compute_metrics(results: dict, lpips_fn) -> torch.Tensor:
    """summarize_dtu.py:21-46: (3, n_seeds) = (lpips, ssim, psnr) per seed, each the mean over all views of
    `imgs_pred * masks` against `imgs_gt * masks`"""
    imgs_gt, masks = results["imgs_gt"], results["masks"]
    assert imgs_gt.shape == masks.shape
    preds = list(results["imgs_pred"])
    gt_m = imgs_gt * masks
    if hasattr(lpips_fn, "compare"):
        lp = lpips_fn.compare(torch.stack([p * masks for p in preds]) * 2 - 1, gt_m * 2 - 1)
        lpips_ = [lp[i].mean().item() for i in range(len(preds))]
    else:
        lpips_ = [lpips_fn_batch(p * masks, gt_m, lpips_fn=lpips_fn).mean().item() for p in preds]
    ssim_, psnr_ = [], []
    for imgs_pred in preds:
        ssim_.append(ssim_fn_batch(imgs_pred * masks, gt_m).mean().item())
        bs = len(imgs_pred)
        mse_b = ((gt_m - imgs_pred * masks) ** 2).view(bs, -1).sum(-1) / masks.view(bs, -1).sum(dim=-1)
        psnr_.append(mse_to_psnr(mse_b).mean().item())
    return torch.from_numpy(np.stack((lpips_, ssim_, psnr_)))


def results_file(run_dir: Path, iteration: int) -> Path:
    """inference/results_all_iter_{it}.pt (the reference's name) or results_all_iter_{it}_*.pt (scripts/inference.py)"""
    inf = Path(run_dir) / "inference"
    found = sorted(set(glob.glob(str(inf / f"results_all_iter_{iteration}.pt")) +
                       glob.glob(str(inf / f"results_all_iter_{iteration}_*.pt"))))
    if len(found) != 1:
        raise FileNotFoundError(f"{inf}: expected one results_all_iter_{iteration}[_*].pt, found {found or 'none'}")
    return Path(found[0])


def load_results(path: Path) -> List[dict]:
    """the result dicts of one file: {object key: result} (key None outside learnable mode 3) or a bare result"""
    obj = torch.load(path, map_location="cpu", weights_only=False)
    if isinstance(obj, dict) and "imgs_gt" in obj:
        return [obj]
    return list(obj.values())


def summarize(runs: Sequence, iterations: Sequence[int], lpips_fn, out=None) -> List[dict]:
    """summarize_dtu.py:48-80: one row per (dtu_subset, iteration, seed), the metrics averaged over the runs (and the
    evaluated objects of a mode-3 run) that share the subset.  Writes `out` as CSV when given."""
    from .inference_dtu import load_train_cfg
    groups: Dict[Tuple[int, int], List[torch.Tensor]] = {}
    for run in runs:
        for it in iterations:
            subset = int(load_train_cfg(Path(run), it).data.dtu_subset)
            for res in load_results(results_file(run, it)):
                groups.setdefault((subset, int(it)), []).append(compute_metrics(res, lpips_fn))
    rows = []
    for subset, it in sorted(groups, key=lambda k: (k[0], list(iterations).index(k[1]))):
        ms = groups[(subset, it)]
        if len({m.shape for m in ms}) != 1:
            raise ValueError(f"dtu_subset {subset}, iteration {it}: the runs were evaluated with different seed counts")
        mean = torch.stack(ms).mean(0)  # (3, n_seeds)
        for seed in range(mean.shape[1]):
            rows.append(dict(num_imgs=subset, dtu_subset=subset, iteration=it, seed=seed, lpips=mean[0, seed].item(),
                             ssim=mean[1, seed].item(), psnr=mean[2, seed].item()))
    if out is not None:
        with open(out, "w", newline="") as f:
            w = csv.DictWriter(f, fieldnames=COLUMNS)
            w.writeheader()
            w.writerows(rows)
    return rows


def expand_runs(patterns: Sequence[str]) -> List[Path]:
    """run directories or globs of them, in sorted order"""
    runs = []
    for p in patterns:
        hits = sorted(glob.glob(p)) if any(c in p for c in "*?[") else [p]
        if not hits:
            raise FileNotFoundError(f"no run directory matches {p!r}")
        runs += [Path(h) for h in hits]
    return runs


def main(argv=None, lpips_fn=None) -> List[dict]:
    import argparse
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--runs", nargs="+", required=True, help="run directories or globs of them")
    ap.add_argument("--iterations", nargs="+", type=int, default=[1500, 3000])
    ap.add_argument("--lpips_vgg_weights", help="torchvision vgg16-397923af.pth")
    ap.add_argument("--lpips_lin_weights", help="lpips weights/v0.1/vgg.pth")
    ap.add_argument("--out", default="summarize_dtu.csv")
    a = ap.parse_args(argv)
    if lpips_fn is None:
        if not (a.lpips_vgg_weights and a.lpips_lin_weights):
            ap.error("--lpips_vgg_weights and --lpips_lin_weights are required (LPIPS is one of the three metrics)")
        from .lpips import LPIPS
        lpips_fn = LPIPS.from_files(a.lpips_vgg_weights, a.lpips_lin_weights)
    rows = summarize(expand_runs(a.runs), a.iterations, lpips_fn, a.out)
    for r in rows:
        print(",".join(str(r[c]) for c in COLUMNS))
    return rows
