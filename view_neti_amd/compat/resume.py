"""Host side of resumable training (extension): everything `Coach` needs beyond the engine's tensors to
continue a run as if it had never stopped — pure functions, no GPU.

  * `ResumableBatchSampler`: the batches of `DataLoader(shuffle=True, drop_last=True)`, draw for draw, with the epoch's
    permutation and the position inside it kept where a checkpoint can reach them;
  * `capture_host_state` / `restore_host_state`: torch's global CPU generator, numpy's global stream (the mode-3 scene
    sampler), python's `random` (caption templates), the loader's generator (world > 1), the sampler, the dataset's scene;
  * checkpoint names: `mapper-steps-N[_object.pt|_view.pt]` -> N, the files a resume from N needs, the newest complete state;
  * `fingerprint` / `check_fingerprint`: what must not differ between the run that saved and the run that resumes;
  * `atomic_save` / `prune_states`: write to a temporary name + `os.replace`, keep the newest K states.

The reference never delivered this (training/coach.py:500-506 raises NotImplementedError; it would not have saved the
optimizer, and its `int(stem.split("-")[-1])` cannot read the `_object` / `_view` names its own CheckpointHandler writes).

Everything stored is tensors, ints, floats, strings, lists, tuples and dicts: a state file loads with
`torch.load(..., weights_only=True)`.
"""
from __future__ import annotations

import os
import random
import re
from pathlib import Path
from typing import Any, Dict, List, Optional, Tuple

import numpy as np
import torch

FORMAT = 1
_MAPPER_RE = re.compile(r"^mapper-steps-(\d+)(?:_object\.pt|_view\.pt)?$")
_STATE_RE = re.compile(r"^trainer-state-steps-(\d+)(?:\.host-rank(\d+))?\.pt$")


# ---------------------------------------------------------------------------------------------- batch order
class ResumableBatchSampler(torch.utils.data.Sampler):
    """`BatchSampler(RandomSampler(range(n), generator=generator), batch_size, drop_last=True)` with its state in reach.

    The draws are RandomSampler's, in its order and at its moments (all lazily, inside the first / last `next()`):
    without a generator one int64 seed from the GLOBAL generator for a private one, then `randperm(n)` for the epoch, and
    when the epoch is exhausted a second `randperm(n)` whose `[:0]` slice is thrown away — that one advances an explicit
    generator, so it is repeated here.  `pos` counts the batches handed out: while the consumer works on batch k the
    generator is suspended behind its `yield` and `pos == k`."""

    def __init__(self, n: int, batch_size: int, generator: Optional[torch.Generator] = None):
        self.n, self.batch_size, self.generator = int(n), int(batch_size), generator
        self.order: Optional[torch.Tensor] = None  # this epoch's permutation of range(n)
        self.pos = 0                               # batches of `order` handed out
        self.epoch = 0                             # permutations drawn so far
        self._resumed = False

    def __len__(self) -> int:
        return self.n // self.batch_size

    def __iter__(self):
        if self._resumed:
            # continue the restored epoch: its permutation was drawn by the run that saved it.  The private generator of
            # the generator=None case is gone, and nothing observable is lost with it (only the discarded tail draw)
            self._resumed = False
            g = self.generator
        else:
            if self.generator is None:
                seed = int(torch.empty((), dtype=torch.int64).random_().item())
                g = torch.Generator()
                g.manual_seed(seed)
            else:
                g = self.generator
            self.order = torch.randperm(self.n, generator=g)
            self.pos = 0
            self.epoch += 1
        order, bs = self.order.tolist(), self.batch_size
        while self.pos < len(self):
            k = self.pos
            self.pos += 1
            yield order[k * bs:(k + 1) * bs]
        if g is not None:
            torch.randperm(self.n, generator=g)

    def state_dict(self) -> Dict[str, Any]:
        order = self.order if self.order is not None else torch.empty(0, dtype=torch.int64)
        return {"order": order.clone(), "pos": int(self.pos), "epoch": int(self.epoch), "n": self.n,
                "batch_size": self.batch_size}

    def load_state_dict(self, sd: Dict[str, Any]):
        if int(sd["n"]) != self.n or int(sd["batch_size"]) != self.batch_size:
            raise ValueError(f"sampler state is for {sd['n']} items in batches of {sd['batch_size']}, this run has "
                             f"{self.n} in batches of {self.batch_size}")
        self.pos, self.epoch = int(sd["pos"]), int(sd["epoch"])
        self._resumed = sd["order"].numel() == self.n and self.epoch > 0
        self.order = sd["order"].clone() if self._resumed else None


# ---------------------------------------------------------------------------------------------- host RNG streams
def capture_host_state(sampler: ResumableBatchSampler, dataset=None,
                       generator: Optional[torch.Generator] = None) -> Dict[str, Any]:
    kind, keys, pos, has_gauss, cached = np.random.get_state()
    if kind != "MT19937":
        raise RuntimeError(f"numpy's global stream is a {kind}, expected MT19937")
    version, internal, gauss_next = random.getstate()
    return {
        "torch": torch.get_rng_state().clone(),
        "numpy": {"keys": torch.from_numpy(keys.astype(np.int64)), "pos": int(pos), "has_gauss": int(has_gauss),
                  "cached_gaussian": float(cached)},
        "python": {"version": int(version), "internal": torch.tensor(internal, dtype=torch.int64),
                   "gauss_next": None if gauss_next is None else float(gauss_next)},
        "generator": generator.get_state().clone() if generator is not None else None,
        "sampler": sampler.state_dict(),
        "current_object_idx": int(getattr(dataset, "current_object_idx", -1)),
    }


def restore_host_state(state: Dict[str, Any], sampler: ResumableBatchSampler, dataset=None,
                       generator: Optional[torch.Generator] = None):
    if (state["generator"] is None) != (generator is None):
        raise ValueError("the saved host state and this run disagree on whether the loader has a generator of its own "
                         "(world size 1 against > 1)")
    sampler.load_state_dict(state["sampler"])
    torch.set_rng_state(state["torch"])
    n = state["numpy"]
    np.random.set_state(("MT19937", n["keys"].numpy().astype(np.uint32), n["pos"], n["has_gauss"], n["cached_gaussian"]))
    p = state["python"]
    random.setstate((p["version"], tuple(int(x) for x in p["internal"].tolist()), p["gauss_next"]))
    if generator is not None:
        generator.set_state(state["generator"])
    if dataset is not None and state["current_object_idx"] >= 0:
        dataset.current_object_idx = state["current_object_idx"]


# ---------------------------------------------------------------------------------------------- names
def parse_step(path) -> int:
    """N of `mapper-steps-N`, `mapper-steps-N_object.pt` or `mapper-steps-N_view.pt`; anything else (`mapper-final`
    included: a finished run has nothing to resume) raises."""
    m = _MAPPER_RE.match(Path(path).name)
    if m is None:
        raise ValueError(f"'{Path(path).name}' is not a step checkpoint: expected mapper-steps-N, mapper-steps-N_object.pt "
                         "or mapper-steps-N_view.pt")
    return int(m.group(1))


def mapper_files(directory, step: int, learnable_mode: int) -> Dict[str, Path]:
    """the mapper checkpoints this mode TRAINS (and therefore saves): object in every mode but 1, view in modes 1-3 (the
    view mapper of modes 4 / 5 is frozen and comes from `model.pretrained_view_mapper`)"""
    d, out = Path(directory), {}
    if learnable_mode != 1:
        out["object"] = d / f"mapper-steps-{step}_object.pt"
    if learnable_mode in (1, 2, 3):
        out["view"] = d / f"mapper-steps-{step}_view.pt"
    return out


def ema_name(name: str) -> str:
    """the name under which the EMA of the mappers is saved beside `mapper-*`: mapper-steps-N.pt ->
    mapper-ema-steps-N.pt, mapper-final.pt -> mapper-ema-final.pt, with or without the _object / _view ending"""
    if not name.startswith("mapper-") or name.startswith("mapper-ema-"):
        raise ValueError(f"'{name}' is not the name of a raw mapper checkpoint")
    return "mapper-ema-" + name[len("mapper-"):]


def ema_mapper_files(directory, step: int, learnable_mode: int) -> Dict[str, Path]:
    """`mapper_files` of the averaged mappers; a frozen view mapper (modes 4 / 5) is not in the bucket and has none"""
    return {k: f.with_name(ema_name(f.name)) for k, f in mapper_files(directory, step, learnable_mode).items()}


def state_file(directory, step: int, rank: int = 0) -> Path:
    name = f"trainer-state-steps-{step}.pt" if rank == 0 else f"trainer-state-steps-{step}.host-rank{rank}.pt"
    return Path(directory) / name


def resume_files(directory, step: int, learnable_mode: int, world: int = 1) -> List[Path]:
    """every file an EXACT resume from step N reads (a warm start needs the mapper files only)"""
    return list(mapper_files(directory, step, learnable_mode).values()) + \
        [state_file(directory, step, r) for r in range(world)]


def resolve_checkpoint(path, learnable_mode: int) -> Tuple[Path, int]:
    """`model.mapper_checkpoint_path` (either file of the pair, or their common stem) -> (directory, N); raises when the
    name is not a step checkpoint or a mapper file of this mode is missing"""
    p = Path(path)
    step = parse_step(p)
    missing = [str(f) for f in mapper_files(p.parent, step, learnable_mode).values() if not f.is_file()]
    if missing:
        raise FileNotFoundError(f"mapper_checkpoint_path '{p}': missing {missing}")
    return p.parent, step


def load_state(path) -> Dict[str, Any]:
    sd = torch.load(path, map_location="cpu", weights_only=True)
    if not isinstance(sd, dict) or sd.get("format") != FORMAT:
        raise ValueError(f"{path}: not a trainer state of format {FORMAT}")
    return sd


def list_states(directory) -> List[int]:
    """steps N that have a `trainer-state-steps-N.pt`, ascending"""
    d = Path(directory)
    if not d.is_dir():
        return []
    steps = []
    for f in d.iterdir():
        m = _STATE_RE.match(f.name)
        if m is not None and m.group(2) is None:
            steps.append(int(m.group(1)))
    return sorted(steps)


def latest_complete_state(directory, learnable_mode: int, world: int = 1) -> Optional[int]:
    """the newest N whose state is whole: every file of `resume_files` exists and the trainer-state files load (a save cut
    short, a truncated copy, a mapper file removed by hand: the state before it is taken)"""
    for step in reversed(list_states(directory)):
        files = resume_files(directory, step, learnable_mode, world)
        if not all(f.is_file() for f in files):
            continue
        try:
            for r in range(world):
                load_state(state_file(directory, step, r))
        except Exception:  # unreadable in any way: torch raises RuntimeError / EOFError / UnpicklingError / ValueError
            continue
        return step
    return None


def atomic_save(obj, path):
    """an interrupted save never leaves a half-written file under the final name"""
    path = Path(path)
    tmp = path.with_name(f".{path.name}.{os.getpid()}.tmp")
    try:
        torch.save(obj, tmp)
        os.replace(tmp, path)
    finally:
        if tmp.exists():
            tmp.unlink()


def prune_states(directory, keep: int) -> List[Path]:
    """remove all but the newest `keep` trainer states (0 = keep all), per-rank host files included; mapper checkpoints
    are never touched.  -> the files removed"""
    if keep <= 0:
        return []
    d = Path(directory)
    old = set(list_states(d)[:-keep])
    removed = []
    for f in sorted(d.iterdir()):
        m = _STATE_RE.match(f.name)
        if m is not None and int(m.group(1)) in old:
            f.unlink()
            removed.append(f)
    return removed


# ---------------------------------------------------------------------------------------------- fingerprint
def fingerprint(learnable_mode: int, batch_size: int, grad_accum: int, world: int, precision: str, seed: Optional[int],
                dataset_len: int, n_params: Optional[int] = None, max_grad_norm: Optional[float] = None,
                snr_gamma: Optional[float] = None, noise_offset: Optional[float] = None, ema_decay: Optional[float] = None,
                ema_update_after_step: int = 0, ema_warmup_power: Optional[float] = None, loss_mask: bool = False,
                loss_mask_background: float = 0.0) -> Dict[str, Any]:
    fp = {"learnable_mode": int(learnable_mode), "train_batch_size": int(batch_size),
          "gradient_accumulation_steps": int(grad_accum), "world_size": int(world), "precision": str(precision),
          "seed": -1 if seed is None else int(seed), "dataset_len": int(dataset_len)}
    if n_params is not None:
        fp["n_params"] = int(n_params)
    if max_grad_norm is not None:  # only when set: the fingerprint of an unclipped run is the one it always was
        fp["max_grad_norm"] = float(max_grad_norm)
    if snr_gamma is not None:  # (the same rule for the objective's options)
        fp["snr_gamma"] = float(snr_gamma)
    if noise_offset is not None:
        fp["noise_offset"] = float(noise_offset)
    if ema_decay is not None:  # (and for the average of the mappers)
        fp["ema_decay"] = float(ema_decay)
    if ema_update_after_step:
        fp["ema_update_after_step"] = int(ema_update_after_step)
    if ema_warmup_power is not None:
        fp["ema_warmup_power"] = float(ema_warmup_power)
    if loss_mask:  # (and for the object-masked objective)
        fp["loss_mask"] = True
    if loss_mask_background:
        fp["loss_mask_background"] = float(loss_mask_background)
    return fp


# fields that are present only where they are set: absent on one side and present on the other is a difference too
_WHEN_SET = ("max_grad_norm", "snr_gamma", "noise_offset", "ema_decay", "ema_update_after_step", "ema_warmup_power",
             "loss_mask", "loss_mask_background")


def check_fingerprint(saved: Dict[str, Any], current: Dict[str, Any]):
    """raises a ValueError that lists every field of `current` the saved state disagrees with"""
    diff = [f"{k}: saved {saved.get(k)!r}, this run {v!r}" for k, v in current.items() if saved.get(k) != v]
    diff += [f"{k}: saved {saved[k]!r}, this run None" for k in _WHEN_SET if k in saved and k not in current]
    if diff:
        raise ValueError("this run cannot continue the saved trainer state; they differ in " + "; ".join(diff))
