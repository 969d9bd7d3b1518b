"""Held-out-view diffusion loss during training (extension).

The reference answers "do the mappers generalise to cameras that were not trained on" by rendering the 34 DTU evaluation
views at every validation step (training/validate.py:65-186).  This is the cheap half of that answer: the FORWARD pass of
the train step (training/coach.py:154-211, `TrainStepEngine.eval_losses`) on the ground-truth image of every evaluation
camera, at K fixed timesteps with fixed noise, one MSE per sample — a deterministic number per (camera, timestep) that is
comparable from step to step and splits into the cameras the run trains on and the ones it never saw.

    plan        pure: which (object, camera, timestep) items exist, their split, and how they are packed into batches
    fixed_noise the (eps, noise) of one item, a function of (seed, camera, k) alone
    HeldoutLoss the evaluator a Coach owns: inputs prepared once, `run(step)` appends one line to heldout-loss.jsonl
    offline     the same evaluation of saved checkpoints (scripts/heldout_loss.py)

Nothing here draws from torch's, numpy's or python's global generators: a run with the evaluation on trains bit-identical
mappers to the same run with it off.
"""
from __future__ import annotations

import json
from dataclasses import dataclass
from pathlib import Path
from typing import Dict, List, Optional, Sequence, Tuple

import torch

FILE_NAME = "heldout-loss.jsonl"
OFFLINE_FILE_NAME = "heldout-loss-offline.jsonl"


@dataclass(frozen=True)
class Item:
    obj: Optional[str]  # the object token (mode 1: the fixed word) the caption names
    cam: int            # DTU camera index (mode 0: index of the training image)
    k: int              # which of the K timesteps
    timestep: int
    split: str          # "train" or "test"


@dataclass
class Plan:
    timesteps: List[int]
    cams: List[int]
    cams_train: List[int]
    cams_test: List[int]
    batches: Dict[Optional[str], List[Tuple[List[Item], int]]]  # object -> [(B items, number of real ones)]

    def n_items(self, obj) -> int:
        return sum(n for _, n in self.batches[obj])


def eval_timesteps(K: int, T: int = 1000) -> List[int]:
    """the midpoints of K equal slices of [0, T): t_k = floor((2k + 1) T / (2K))"""
    if K < 1:
        raise ValueError("heldout_loss_timesteps must be >= 1")
    return [((2 * k + 1) * T) // (2 * K) for k in range(K)]


def noise_seed(seed: int, cam: int, k: int) -> int:
    return seed + 1000 * cam + k


def fixed_noise(seed: int, cam: int, k: int, h: int, w: int, channels: int = 4) -> Tuple[torch.Tensor, torch.Tensor]:
    """(eps, noise) of item (cam, k): `latent_dist.sample()`'s draw first, then the diffusion noise, from one CPU
    generator per item — the values never depend on how the items are batched"""
    g = torch.Generator().manual_seed(noise_seed(seed, cam, k))
    eps = torch.randn((channels, h, w), generator=g)
    noise = torch.randn((channels, h, w), generator=g)
    return eps, noise


def plan(learnable_mode: int, camera_representation: str, dtu_subset: int, objects: Sequence[Optional[str]],
         n_timesteps: int, batch: int, n_train_images: int = 0, T: int = 1000) -> Plan:
    """View modes on dtu-12d: the 34 evaluation cameras of `dtu_metrics.get_cam_idxs(dtu_subset)`, each `train` or
    `test`.  Mode 0 has no cameras: the run's own `n_train_images` training images, all `train`.  Items are
    object x camera x k in that nesting order, packed per object into batches of `batch`; a partial last batch repeats
    its last item (`inference_dtu.plan_batches`) and the extra outputs are dropped."""
    from .inference_dtu import plan_batches
    ts = eval_timesteps(n_timesteps, T)
    if learnable_mode == 0:
        if n_train_images < 1:
            raise ValueError("held-out loss in learnable_mode 0 evaluates the run's own training images: none given")
        cams = list(range(n_train_images))
        train, test = list(cams), []
    else:
        if camera_representation != "dtu-12d":
            raise NotImplementedError("the held-out loss of the view modes is defined for camera_representation 'dtu-12d'")
        from .dtu_metrics import get_cam_idxs
        cams, train, test = get_cam_idxs(dtu_subset)  # (a training view outside the evaluation split is not evaluated)
    is_train = set(train)
    batches = {}
    for obj in objects:
        packed = plan_batches([obj], cams, list(range(len(ts))), batch)
        batches[obj] = [([Item(o, c, k, ts[k], "train" if c in is_train else "test") for o, c, k in entries], n)
                        for entries, n in packed]
    return Plan(ts, list(cams), list(train), list(test), batches)


# ---------------------------------------------------------------------------------------------- records
def _mean(xs: Sequence[float]) -> Optional[float]:
    return float(sum(xs) / len(xs)) if len(xs) else None


def _object_record(p: Plan, rows: List[Tuple[Item, float]]) -> dict:
    sel = lambda split, t=None: [v for it, v in rows if it.split == split and (t is None or it.timestep == t)]
    return {"train": _mean(sel("train")), "test": _mean(sel("test")),
            "by_timestep": {str(t): {"train": _mean(sel("train", t)), "test": _mean(sel("test", t))} for t in p.timesteps},
            "by_view": {str(c): _mean([v for it, v in rows if it.cam == c]) for c in p.cams}}


def make_record(step: int, p: Plan, losses: Dict[Optional[str], List[Tuple[Item, float]]],
                ema_losses: Optional[Dict[Optional[str], List[Tuple[Item, float]]]] = None,
                masked_losses: Optional[Dict[Optional[str], List[Tuple[Item, float]]]] = None) -> dict:
    """{"step", "timesteps", "objects": {tok: {"train", "test", "by_timestep": {t: {"train", "test"}}, "by_view": {cam: m}}}};
    every m is a mean over per-sample losses, None for an empty split.  ema_losses (a run with optim.ema_decay): the same
    plan evaluated with the averaged mappers; each object then gains "ema": {"train", "test", "by_timestep", "by_view"}
    beside the unchanged raw fields.  masked_losses (eval.heldout_loss_masked): the same items' losses under
    the evaluation views' object masks; each object then gains "loss_masked": the four fields again, and "by_view_timestep":
    {cam: {t: value}}, one value per (camera, timestep)"""
    objects = {}
    for obj, rows in losses.items():
        objects[str(obj)] = _object_record(p, rows)
        if ema_losses is not None:
            objects[str(obj)]["ema"] = _object_record(p, ema_losses[obj])
        if masked_losses is not None:
            m = _object_record(p, masked_losses[obj])
            m["by_view_timestep"] = {str(c): {str(it.timestep): v for it, v in masked_losses[obj] if it.cam == c}
                                     for c in p.cams}
            objects[str(obj)]["loss_masked"] = m
    return {"step": int(step), "timesteps": list(p.timesteps), "objects": objects}


def append_record(path, record: dict) -> None:
    with open(path, "a") as f:
        f.write(json.dumps(record) + "\n")


def read_records(path) -> List[dict]:
    """the lines of a heldout-loss jsonl file, with the timestep and camera keys back as ints"""
    out = []
    with open(path) as f:
        for line in f:
            if not line.strip():
                continue
            r = json.loads(line)
            for o in r["objects"].values():
                o["by_timestep"] = {int(t): v for t, v in o["by_timestep"].items()}
                o["by_view"] = {int(c): v for c, v in o["by_view"].items()}
                for sub in ("ema", "loss_masked"):
                    if sub in o:
                        o[sub]["by_timestep"] = {int(t): v for t, v in o[sub]["by_timestep"].items()}
                        o[sub]["by_view"] = {int(c): v for c, v in o[sub]["by_view"].items()}
                if "loss_masked" in o:
                    o["loss_masked"]["by_view_timestep"] = {int(c): {int(t): v for t, v in d.items()}
                                                            for c, d in o["loss_masked"]["by_view_timestep"].items()}
            out.append(r)
    return out


def summary_line(step: int, record: dict) -> str:
    fmt = lambda v: "n/a" if v is None else f"{v:.5f}"
    ema = lambda o: f" (ema: train {fmt(o['ema']['train'])} test {fmt(o['ema']['test'])})" if "ema" in o else ""
    return f"heldout loss step {step}: " + "  ".join(
        f"{tok} train {fmt(o['train'])} test {fmt(o['test'])}{ema(o)}" for tok, o in record["objects"].items())


# ---------------------------------------------------------------------------------------------- the evaluator
class HeldoutLoss:
    """Built by a Coach (rank 0).  Reads the Coach's dataset, tokenizer, camera scaling and engine; the preprocessed
    pixels of the evaluation images and the fixed noise are prepared at the first evaluation and kept."""

    masked = False  # (eval.heldout_loss_masked, set by __init__)

    def __init__(self, coach, n_timesteps: Optional[int] = None, seed: Optional[int] = None, masked: Optional[bool] = None):
        from .inference_dtu import eval_object_token, scene_of
        self.coach = coach
        cfg, ds, eng = coach.cfg, coach.train_dataset, coach.engine
        self.seed = cfg.eval.heldout_loss_seed if seed is None else seed
        K = cfg.eval.heldout_loss_timesteps if n_timesteps is None else n_timesteps
        mode = cfg.learnable_mode
        if mode == 0:
            objects = [ds.placeholder_object_tokens[0]]
        elif mode == 3:
            objects = list(cfg.eval.eval_placeholder_object_tokens or ds.placeholder_object_tokens[:1])
            for t in objects:
                if t not in ds.placeholder_object_tokens:
                    raise ValueError(f"eval_placeholder_object_tokens: {t!r} is not one of the run's tokens "
                                     f"{list(ds.placeholder_object_tokens)}")
        else:
            objects = [eval_object_token(cfg, ds.placeholder_object_tokens)]
        self.plan = plan(mode, cfg.data.camera_representation, cfg.data.dtu_subset, objects, K, eng.B,
                         n_train_images=ds.num_images if mode == 0 else 0, T=coach.sd.ddpm.num_train_timesteps)
        # the image of every (object, camera): checked now, so that a missing ground-truth view stops the run at its
        # construction and not at the first evaluation
        self.image_path: Dict[Tuple[Optional[str], int], Path] = {}
        for obj in objects:
            for cam in self.plan.cams:
                if mode == 0:
                    f = Path(ds.image_paths[cam])
                else:
                    scene, _ = scene_of(cfg, obj if mode == 3 else None)
                    f = scene / ds.dtu_cam_and_lighting_to_fname(cam, cfg.data.dtu_lighting)
                if not f.is_file():
                    raise FileNotFoundError(f"held-out loss: the evaluation image of camera {cam} ({obj}) is missing: {f}")
                self.image_path[(obj, cam)] = f
        # eval.heldout_loss_masked: the evaluation views' object masks at the training resolution; a
        # missing mask file stops the run here as well
        self.masked = bool(cfg.eval.heldout_loss_masked if masked is None else masked)
        self._mask_rows: Dict[Tuple[Optional[str], int], torch.Tensor] = {}
        if self.masked:
            if ds.mask_dir is None:
                raise ValueError("the masked held-out loss needs data.mask_dir")
            for key, f in self.image_path.items():
                if not ds.mask_path(f).is_file():
                    raise FileNotFoundError(f"held-out loss: the object mask of camera {key[1]} ({key[0]}) is missing: "
                                            f"{ds.mask_path(f)}")
            self._weights = torch.ones(eng.B, eng.h * eng.w, dtype=torch.float32, device=eng.dev)
        self._pixels: Dict[Tuple[Optional[str], int], torch.Tensor] = {}
        self._noise: Dict[Tuple[int, int], Tuple[torch.Tensor, torch.Tensor]] = {}
        self._text: Dict[Optional[str], Tuple[torch.Tensor, int, int]] = {}
        self._cams: Dict[int, torch.Tensor] = {}

    # -- inputs, each prepared once
    def pixels(self, obj, cam) -> torch.Tensor:
        key = (obj, cam)
        if key not in self._pixels:
            px = self.coach.train_dataset.load_pixels(self.image_path[key])
            if tuple(px.shape[1:]) != tuple(self.coach.engine.pixel_values.shape[2:]):
                raise ValueError(f"{self.image_path[key]}: preprocessed to {tuple(px.shape[1:])}, the engine trains at "
                                 f"{tuple(self.coach.engine.pixel_values.shape[2:])}")
            self._pixels[key] = px
        return self._pixels[key]

    def mask_row(self, obj, cam) -> torch.Tensor:
        """the loss weights of one evaluation view (f32 device [h*w]): its mask through load_source and `_resize`, no flip,
        no augmentation, then the preparation entry with the run's background weight"""
        from .. import ops
        key = (obj, cam)
        if key not in self._mask_rows:
            eng, ds = self.coach.engine, self.coach.train_dataset
            m = torch.from_numpy(ds.load_mask(self.image_path[key])).to(eng.dev)
            if tuple(m.shape) != (eng.H, eng.W):
                raise ValueError(f"{ds.mask_path(self.image_path[key])}: preprocessed to {tuple(m.shape)}, the engine trains "
                                 f"at {(eng.H, eng.W)}")
            row = torch.empty(1, eng.h * eng.w, dtype=torch.float32, device=eng.dev)
            ws = torch.zeros(ops.loss_weights_from_mask_ws_ints(eng.H, eng.W, eng.vae_factor), dtype=torch.int32,
                             device=eng.dev)
            ops.loss_weights_from_mask(m, eng.H, eng.W, 1, eng.vae_factor, eng.MASK_THRESHOLD,
                                       self.coach.cfg.optim.loss_mask_background, row, 0, ws)
            self._mask_rows[key] = row[0]
        return self._mask_rows[key]

    def noise(self, cam, k) -> Tuple[torch.Tensor, torch.Tensor]:
        if (cam, k) not in self._noise:
            eng = self.coach.engine
            self._noise[(cam, k)] = fixed_noise(self.seed, cam, k, eng.h, eng.w, eng.cfg.vae.latent_channels)
        return self._noise[(cam, k)]

    def caption(self, obj) -> str:
        ds = self.coach.train_dataset
        if self.coach.cfg.learnable_mode == 0:
            return f"A photo of a {obj}"
        return f"{ds.placeholder_view_tokens[0]}. A photo of a {obj}"  # any view placeholder: see camera_params

    def text(self, obj) -> Tuple[torch.Tensor, int, int]:
        """(input ids (L,), object placeholder id or -1, view placeholder id or -1) of the object's caption"""
        if obj not in self._text:
            coach, tok = self.coach, self.coach.tokenizer
            ids = tok(self.caption(obj), padding="max_length", truncation=True, max_length=tok.model_max_length,
                      return_tensors="pt").input_ids[0]
            mode = coach.cfg.learnable_mode
            po = -1 if mode == 1 else int(tok.convert_tokens_to_ids(obj))
            pv = -1 if mode == 0 else int(coach.placeholder_view_token_ids[0])
            self._text[obj] = (ids, po, pv)
        return self._text[obj]

    def camera_params(self, cam) -> torch.Tensor:
        """the engine takes camera PARAMETERS, not token ids, so a held-out camera needs no vocabulary entry: its own 12
        numbers (through the 4-decimal token string, Q15, like every training camera) scaled as Coach._view_params does"""
        if cam not in self._cams:
            ds, mv = self.coach.train_dataset, self.coach.mapper_view
            p = ds.dtu_token_to_cam_params(ds.lookup_camidx_to_view_token[cam])[0]
            self._cams[cam] = (p - mv.cam_mins) / (mv.cam_maxs - mv.cam_mins) * 2 - 1
        return self._cams[cam]

    # -- the evaluation
    def evaluate(self, masked_out: Optional[dict] = None) -> Dict[Optional[str], List[Tuple[Item, float]]]:
        """masked_out: a dict that receives the masked losses of the same items (only with `masked`)"""
        coach, eng = self.coach, self.coach.engine
        has_view = coach.mapper_view is not None
        out = {}
        for obj, batches in self.plan.batches.items():
            ids, po, pv = self.text(obj)
            B = eng.B
            slot = coach.object_slot.get(po, 0)
            rows, mrows = [], []
            for items, n in batches:
                eng.set_batch(torch.stack([self.pixels(obj, it.cam) for it in items]), ids.unsqueeze(0).repeat(B, 1),
                              torch.full((B,), po), torch.full((B,), pv) if has_view else None,
                              torch.stack([self.camera_params(it.cam) for it in items]) if has_view else None,
                              object_index=slot, for_eval=True)
                pairs = [self.noise(it.cam, it.k) for it in items]
                eng.set_noise(torch.stack([e for e, _ in pairs]), torch.stack([z for _, z in pairs]),
                              torch.tensor([it.timestep for it in items], dtype=torch.int64))
                if masked_out is None:
                    losses = eng.eval_losses().tolist()
                else:
                    torch.stack([self.mask_row(obj, it.cam) for it in items], out=self._weights)
                    losses, mlosses = (v.tolist() for v in eng.eval_losses(weights=self._weights))
                    mrows += [(it, mlosses[i]) for i, it in enumerate(items[:n])]
                rows += [(it, losses[i]) for i, it in enumerate(items[:n])]
            out[obj] = rows
            if masked_out is not None:
                masked_out[obj] = mrows
        return out

    def run(self, step: int, file_name: str = FILE_NAME, weights: Optional[str] = None) -> dict:
        """one evaluation -> one line.  An engine that keeps an average of the mappers (optim.ema_decay) runs the plan twice,
        raw and then inside ema_weights().  weights: a note of which saved weights the engine holds (offline, --use_ema)"""
        masked = {} if self.masked else None
        losses, ema_losses = (self.evaluate() if masked is None else self.evaluate(masked)), None
        eng = self.coach.engine
        if eng.ema is not None:
            with eng.ema_weights():
                ema_losses = self.evaluate()
        record = make_record(step, self.plan, losses, ema_losses, masked)
        if weights is not None:
            record["weights"] = weights
        append_record(Path(self.coach.cfg.log.exp_dir) / file_name, record)
        self.coach.log(summary_line(step, record))
        return record


# ---------------------------------------------------------------------------------------------- saved checkpoints
def offline(input_dir, iterations: Sequence[int], eval_placeholder_object_tokens: Sequence[str] = (),
            n_timesteps: int = 4, seed: int = 0, device: str = "cuda", use_ema: bool = False,
            masked: bool = False) -> List[dict]:
    """The same plan, seeds and inputs on the `mapper-steps-N` checkpoints of a finished run: the run's config from the
    first checkpoint (`inference_dtu.load_train_cfg`), ONE forward-only engine, each iteration's mappers copied into it
    in place.  Appends to <input_dir>/heldout-loss-offline.jsonl and returns the records.  use_ema: the averaged mappers
    `mapper-ema-steps-N` of a run with optim.ema_decay instead (a missing file raises); such a line says "weights": "ema".
    masked: "loss_masked" beside every loss, under the object masks of the run's data.mask_dir (which it then needs)."""
    from .coach import Coach
    from .inference_dtu import load_train_cfg
    input_dir = Path(input_dir)
    iterations = [int(i) for i in iterations]
    if not iterations:
        raise ValueError("heldout_loss: no iterations given")
    cfg = load_train_cfg(input_dir, iterations[0])
    cfg.log.exp_dir = input_dir
    if eval_placeholder_object_tokens:
        cfg.eval.eval_placeholder_object_tokens = list(eval_placeholder_object_tokens)
    coach = Coach(cfg, device=device, forward_only=True)
    ev = HeldoutLoss(coach, n_timesteps=n_timesteps, seed=seed, masked=masked)
    records = []
    for it in iterations:
        coach.load_mappers(input_dir, it, ema=use_ema)
        records.append(ev.run(it, OFFLINE_FILE_NAME, weights="ema" if use_ema else None))
    return records


def format_table(records: Sequence[dict]) -> str:
    """iteration x object: train / test means"""
    fmt = lambda v: "n/a".rjust(10) if v is None else f"{v:10.5f}"
    lines = [f"{'iteration':>9}  {'object':<20} {'train':>10} {'test':>10}"]
    for r in records:
        for tok, o in r["objects"].items():
            lines.append(f"{r['step']:>9}  {tok:<20} {fmt(o['train'])} {fmt(o['test'])}")
    return "\n".join(lines)
