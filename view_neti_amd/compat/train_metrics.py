"""`log.train_metrics` (extension): the per-step training record as `<exp_dir>/train-metrics.jsonl`.

The reference logs `total_loss` and `lr` to its tracker after every micro-step (training/coach.py:256-261).  Here the
device writes one ring row per micro-step inside the captured step (engine/step.py, engine/telemetry.py) and the host
fetches the ring where the train loop already syncs; this module turns the rows into one JSON line per optimizer step:

    {"step": 7, "loss": 0.41, "lr": 0.012, "loss_scale": 65536.0, "skipped": false,
     "grad_norm": {"object": 0.8, "view": 0.3, "total": 0.85}, "clip_coef": 1.0,
     "samples": [{"t": 981, "loss": 0.02}, ...]}

`loss` is the mean of the group's per-sample losses: the reference's `total_loss` averaged over the accumulation group.
`samples` has one entry per sample of every micro-step of the group — the loss-by-timestep curve is read off these.  A side
of `grad_norm` that the run does not train is omitted (mode 1: no object mapper; mode 5: a frozen view mapper); a non-finite
norm (a skipped step) is null.  A run with `optim.snr_gamma` (§9 f8) has one more key, `"loss_weighted"`: the Min-SNR
weighted mean of the same samples — the quantity the step minimises — computed here in f64 from the (t, loss) pairs and the
f32 `alphas_cumprod` table; `loss` stays the unweighted mean, so files of weighted and unweighted runs compare.  A run with
`data.mask_dir` (§9 f11) says `"masked": true`: its per-sample losses, and every mean over them, are the object-masked
ones.  Pure functions and a small file writer: no GPU."""
from __future__ import annotations

import json
import os
from pathlib import Path
from typing import Dict, List, Optional, Sequence, Tuple

from ..engine.telemetry import finite_or_none

FILE_NAME = "train-metrics.jsonl"
LOG_EVERY = 50  # the train loop's text line, where it syncs anyway


def group_rows(rows: List[Dict]) -> Tuple[List[List[Dict]], List[Dict], int]:
    """micro-step rows, oldest first -> (whole accumulation groups, the rows of a group still open at the end, rows
    dropped).  A group is whole when its rows carry the micro indices 0, 1, ..., k on consecutive micro-steps and the last
    one closed the group; rows of a group whose beginning the ring has lost are dropped."""
    groups, cur, dropped = [], [], 0
    for r in rows:
        follows = cur and r["micro"] == cur[-1]["micro"] + 1 and r["micro_step"] == cur[-1]["micro_step"] + 1
        if r["micro"] == 0 or not follows:
            dropped += len(cur)
            cur = []
        if r["micro"] != 0 and not cur:
            dropped += 1
            continue
        cur.append(r)
        if r["closed"]:
            groups.append(cur)
            cur = []
    return groups, cur, dropped


def min_snr_weight(alpha_cumprod: float, gamma: float, v_prediction: bool = False) -> float:
    """Min-SNR-gamma weight of one timestep in f64: snr = a / (1 - a); min(snr, gamma) / snr, or / (snr + 1) for
    v-prediction (the formula of vneti_mse_loss_grad_snr, include/vneti.h)"""
    a = float(alpha_cumprod)
    snr = a / (1.0 - a)
    return min(snr, float(gamma)) / (snr + 1.0 if v_prediction else snr)


def step_line(step: int, group: List[Dict], omit_object: bool = False, omit_view: bool = False,
              snr_gamma: Optional[float] = None, alphas_cumprod: Optional[Sequence[float]] = None,
              v_prediction: bool = False, masked: bool = False) -> Dict:
    """one optimizer step's line from the rows of its accumulation group (the last row closed it).  snr_gamma set: the
    line gains "loss_weighted" (alphas_cumprod: the f32 table, indexable by timestep).  masked: the rows' losses are the
    object-masked ones; the line says "masked": true"""
    last = group[-1]
    assert last["closed"], "the group's last micro-step did not close it"
    samples = [{"t": t, "loss": l} for r in group for t, l in zip(r["timesteps"], r["losses"])]
    norm = {k: finite_or_none(v) for k, v in last["grad_norm"].items()
            if not (k == "object" and omit_object) and not (k == "view" and omit_view)}
    norm = {k: norm[k] for k in ("object", "view", "total") if k in norm}
    line = {"step": int(step), "loss": finite_or_none(sum(s["loss"] for s in samples) / len(samples)), "lr": last["lr"],
            "loss_scale": last["loss_scale"], "skipped": bool(last["skipped"]), "grad_norm": norm,
            "clip_coef": last["clip_coef"], "samples": [{"t": s["t"], "loss": finite_or_none(s["loss"])} for s in samples]}
    if snr_gamma is not None:
        if alphas_cumprod is None:
            raise ValueError("step_line(): snr_gamma needs the alphas_cumprod table")
        w = [min_snr_weight(alphas_cumprod[int(s["t"])], snr_gamma, v_prediction) for s in samples]
        line["loss_weighted"] = finite_or_none(sum(wi * float(s["loss"]) for wi, s in zip(w, samples)) / len(samples))
    if masked:
        line["masked"] = True
    return line


def lines_up_to(groups: List[List[Dict]], step: int, **kw) -> List[Dict]:
    """the groups are the LAST len(groups) optimizer steps up to and including `step`; kw: step_line's options"""
    first = step - len(groups) + 1
    return [step_line(first + i, g, **kw) for i, g in enumerate(groups)]


def truncate_file(path, step: int) -> int:
    """keep the lines with "step" <= step (a resume from step N continues the file at N + 1; a fresh run, step 0, starts
    it empty); an unreadable last line — a write cut short — goes too.  -> lines kept"""
    path = Path(path)
    kept = []
    if path.is_file():
        for line in path.read_text().splitlines():
            try:
                if int(json.loads(line)["step"]) <= step:
                    kept.append(line)
            except (ValueError, KeyError, TypeError):
                continue
    tmp = path.with_name(f".{path.name}.{os.getpid()}.tmp")
    tmp.write_text("".join(l + "\n" for l in kept))
    os.replace(tmp, path)
    return len(kept)


class TrainMetricsFile:
    """appends lines; opened on a resume from step N it first drops what a previous run wrote past N"""

    def __init__(self, exp_dir, start_step: int = 0):
        self.path = Path(exp_dir) / FILE_NAME
        self.path.parent.mkdir(parents=True, exist_ok=True)
        self.kept = truncate_file(self.path, start_step)
        self.last = None  # the newest line written by this run

    def append(self, lines: List[Dict]):
        if not lines:
            return
        with self.path.open("a") as f:
            for d in lines:
                f.write(json.dumps(d) + "\n")
        self.last = lines[-1]
