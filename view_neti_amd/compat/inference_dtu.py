"""DTU novel-view evaluation of a trained run — the reference's training/inference_dtu.py:88-280
(`dtu_generate_camidxs_to_preds`) and scripts/inference.py:34-135 (`InferenceConfig`, `main`), batched.

The reference renders one prompt per sampler run: 34 evaluation views x seeds x evaluated objects B = 1 calls.  Here
every (object, camera, seed) triple is one sample of a batch of B different prompts (`sd_pipeline_call` with a list of
PromptEmbeds and a list of generators): sample i starts from randn((1, 4, h, w), Generator().manual_seed(seed_i)), the
draw of the B = 1 call, and each sample picks its own object mapper of the run's bucket (vneti_mapper_fwd_slots).  A
partial last batch repeats its last entry and drops the extra outputs, so one captured sampler graph serves the whole
evaluation.

    preds = dtu_generate_camidxs_to_preds(train_cfg, cam_idxs, step=1500, seeds=[0, 1], batch=8)
"""
from __future__ import annotations

from dataclasses import dataclass, field
from pathlib import Path
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from .. import sd_config as sc
from . import config as cfgmod
from .checkpoint_handler import CheckpointHandler
from .coach import _sd_family
from .dataset import TextualInversionDataset

Entry = Tuple[Optional[str], int, int]  # (object token, camera index, seed)


@dataclass
class InferenceConfig:
    """scripts/inference.py:34-57 of the reference (+ `batch`: prompts per sampler run)"""
    iteration: Optional[int] = None
    input_dir: Optional[Path] = None
    inference_dir: Optional[Path] = None
    seeds: List[int] = field(default_factory=lambda: [42])
    eval_placeholder_object_tokens: List[str] = field(default_factory=lambda: [])
    torch_dtype: str = "fp16"
    num_denoising_steps: int = 30
    debug: int = 0
    batch: int = 8
    # LPIPS(net="vgg") on the GPU from the user's weight files (compat/lpips.py); off by default, as in the reference
    do_lpips: bool = False
    lpips_vgg_weights: Optional[Path] = None
    lpips_lin_weights: Optional[Path] = None
    # evaluate the averaged mappers mapper-ema-steps-N_* of a run with optim.ema_decay instead of the raw ones
    use_ema: bool = False
    # Lin et al. 2023 for v-prediction models sampled with guidance: diffusers' guidance_rescale in [0, 1]
    # and the schedulers' timestep_spacing (None | "trailing"); both off by default
    guidance_rescale: float = 0.0
    timestep_spacing: Optional[str] = None

    def __post_init__(self):
        from ..engine.infer import check_rescale, inference_timesteps
        check_rescale(self.guidance_rescale)
        inference_timesteps("ddim", 1, spacing=self.timestep_spacing)  # a bad string raises here, not after the load
        if self.do_lpips and (self.lpips_vgg_weights is None or self.lpips_lin_weights is None):
            raise ValueError("do_lpips needs --lpips_vgg_weights (torchvision vgg16-397923af.pth) and "
                             "--lpips_lin_weights (lpips weights/v0.1/vgg.pth)")
        if self.do_lpips and self.torch_dtype == "bf16":
            raise ValueError("do_lpips: LPIPS runs on the fp16 library only (its bf16 quality is unmeasured)")
        if self.input_dir is not None and self.inference_dir is None:
            self.inference_dir = Path(self.input_dir) / "inference"
        if self.torch_dtype not in ("fp16", "bf16"):
            # like Coach with mixed_precision "no": the engines have no fp32 path
            raise ValueError(f"torch_dtype {self.torch_dtype!r}: the HIP engines run fp16 (or bf16) only")
        if self.batch < 1:
            raise ValueError("batch must be >= 1")


def parse_inference_config(args: Optional[List[str]] = None) -> InferenceConfig:
    """`--config_path inference.yaml` plus dotted overrides (`--iteration 1500 --seeds [0,1]`), as pyrallis does"""
    cfg = cfgmod.parse(InferenceConfig, args)
    if cfg.input_dir is None or cfg.iteration is None:
        raise SystemExit("inference: input_dir and iteration are required")
    return cfg


def nvs_resolution(train_cfg, sd: sc.SDConfig) -> Tuple[int, int]:
    """(height, width) of the novel views (inference_dtu.py:238-240): 768 x 576 for dtu_preprocess_key 1.  For key 0
    the reference sets no size and fails with UnboundLocalError at :256; here key 0 renders at the UNet's default size
    (768^2 for SD-2.1, 512^2 for SD-1.x), which on SD-2.1 is the 768^2 key-0 ground truth of dtu_get_gt_images."""
    key = train_cfg.data.dtu_preprocess_key
    if key == 1:
        return 576, 768
    if key == 0:
        s = 768 if sd.name == "sd21" else 512
        return s, s
    raise NotImplementedError(f"dtu_preprocess_key {key}")


def eval_object_token(train_cfg, placeholder_object_tokens: Sequence[str],
                      eval_placeholder_object_token: Optional[str] = None) -> str:
    """inference_dtu.py:218-229: the evaluation token (mode 3), the learned token (pretrained object, modes 2/4/5), or
    the fixed word (mode 1)"""
    if eval_placeholder_object_token:
        tok = eval_placeholder_object_token
    elif "/" in str(train_cfg.data.fixed_object_token_or_path) or train_cfg.learnable_mode in (2, 4, 5):
        tok = placeholder_object_tokens[0]
    else:
        tok = train_cfg.data.fixed_object_token_or_path
    if train_cfg.learnable_mode != 1 and tok not in placeholder_object_tokens:
        raise ValueError(f"object token {tok!r} is not one of the run's tokens {list(placeholder_object_tokens)}")
    return tok


def plan_batches(objects: Sequence[Optional[str]], cam_idxs: Sequence[int], seeds: Sequence[int],
                 batch: int) -> List[Tuple[List[Entry], int]]:
    """(object, camera, seed) in that nesting order, cut into batches of `batch`; a partial last batch repeats its last
    entry up to the full size.  -> [(entries, number of real entries)]"""
    items = [(o, c, s) for o in objects for c in cam_idxs for s in seeds]
    out = []
    for i in range(0, len(items), batch):
        chunk = items[i:i + batch]
        n = len(chunk)
        out.append((chunk + [chunk[-1]] * (batch - n), n))
    return out


def preds_png_name(token, iteration, seed) -> str:
    return f"preds_object_{token}_iter_{iteration}_seed{seed}.png"


def results_name(iteration, tokens, seeds) -> str:
    return f"results_all_iter_{iteration}_scans_{list(tokens)}_seeds_{list(seeds)}.pt"


def prompt_for(view_token: str, object_token: str) -> str:
    return f"{view_token}. A photo of a {object_token}"


def generate_views(pipe, pm, objects: Sequence[str], cam_idxs: Sequence[int], seeds: Sequence[int],
                   num_denoising_steps: int, guidance_scale: float = 7.5,
                   guidance_rescale: float = 0.0) -> Dict[str, Dict[int, np.ndarray]]:
    """object -> camidx -> uint8 (n_seeds, H, W, 3), all triples through batches of the engine's size (the timestep
    spacing is the pipeline's, `pipe.timestep_spacing`)"""
    from .sd_pipeline_call import sd_pipeline_call
    lut, _ = TextualInversionDataset.dtu_generate_dset_cam_tokens_params()
    B = pipe.engine.B
    imgs: Dict[Entry, np.ndarray] = {}
    embeds = {}
    for entries, n in plan_batches(objects, cam_idxs, seeds, B):
        prompts = []
        for o, c, _ in entries:
            if (o, c) not in embeds:
                embeds[(o, c)] = pm.embed_prompt(prompt_for(lut[c], o))
            prompts.append(embeds[(o, c)])
        gens = [torch.Generator().manual_seed(s) for _, _, s in entries]
        # always the per-sample form (also at B = 1): it is what writes each sample's object slot
        out = sd_pipeline_call(pipe, prompts, num_inference_steps=num_denoising_steps, guidance_scale=guidance_scale,
                               generator=gens, num_images_per_prompt=B, output_type="np", return_dict=False,
                               guidance_rescale=guidance_rescale)[0]
        u8 = (out * 255).round().astype(np.uint8)
        for k in range(n):
            imgs[entries[k]] = u8[k]
    return {o: {c: np.stack([imgs[(o, c, s)] for s in seeds]) for c in cam_idxs} for o in objects}


def nvs_mapper_stems(input_dir, step: int, learnable_mode: int, use_ema: bool = False) -> Tuple[str, str]:
    """(object stem, view stem) of the checkpoint files the evaluation of iteration `step` loads.  use_ema: the averaged
    mappers `mapper-ema-steps-N_*` for every mapper the run trained — a missing one raises naming it, the raw file is never
    taken in its place; a frozen view mapper (modes 4 / 5) has no average and stays the raw file"""
    from . import resume
    raw = f"mapper-steps-{step}"
    if not use_ema:
        return raw, raw
    files = resume.ema_mapper_files(input_dir, step, learnable_mode)
    missing = [str(f) for f in files.values() if not f.is_file()]
    if missing:
        raise FileNotFoundError(f"use_ema: iteration {step} has no averaged mappers: missing {missing} (they are written "
                                "by runs with optim.ema_decay)")
    ema = resume.ema_name(raw)
    return (ema if "object" in files else raw), (ema if "view" in files else raw)


def load_nvs_pipeline(train_cfg, step: int, batch: int, device: str = "cuda", use_ema: bool = False):
    """the run's mappers at `step` (mapper-steps-{step}_{view,object}.pt, inference_dtu.py:119-123), every object
    mapper in one per-sample bucket, at the novel-view resolution"""
    from .inference import build_inference
    h, w = nvs_resolution(train_cfg, _sd_family(train_cfg))
    exp_dir = Path(train_cfg.log.exp_dir)
    obj_stem, view_stem = nvs_mapper_stems(exp_dir, step, train_cfg.learnable_mode, use_ema)
    return build_inference(train_cfg, exp_dir, obj_stem, batch, h, w, device=device, per_sample=True, view_stem=view_stem)


def dtu_generate_camidxs_to_preds(train_cfg, cam_idxs, step, num_denoising_steps: int = 30,
                                  seeds: Sequence[int] = (0, 1), eval_placeholder_object_token: Optional[str] = None,
                                  guidance_scale: float = 7.5, batch: int = 8, pipeline=None
                                  ) -> Dict[int, np.ndarray]:
    """inference_dtu.py:88-280: camidx -> uint8 (n_seeds, H, W, 3) for one object token.  `pipeline` = (pipe, pm) of
    load_nvs_pipeline to reuse across calls."""
    pipe, pm = pipeline or load_nvs_pipeline(train_cfg, step, batch)
    tokens = pipe.object_tokens
    obj = eval_object_token(train_cfg, tokens, eval_placeholder_object_token)
    return generate_views(pipe, pm, [obj], list(cam_idxs), list(seeds), num_denoising_steps, guidance_scale)[obj]


def scene_of(train_cfg, object_token: Optional[str]) -> Tuple[Path, str]:
    """the ground-truth scene directory and scan id of an evaluated object (mode 3: `<scanN>` tokens under the data
    root; otherwise the run's own scene)"""
    if train_cfg.learnable_mode == 3 and object_token:
        scan_id = object_token[5:-1]
        return Path(train_cfg.data.train_data_dir) / f"scan{scan_id}", scan_id
    root = Path(train_cfg.data.train_data_dir)
    return root, root.stem[4:]


def evaluate(train_cfg, per_cam: Dict[int, np.ndarray], seeds: Sequence[int], object_token: Optional[str],
             make_figures: bool = True, lpips_fn=None) -> dict:
    """validate.py:123-152: masked MSE / PSNR / SSIM of the views against the scene, and LPIPS when an `lpips_fn`
    (compat/lpips.py) is given (otherwise its entries stay 0, the reference's do_lpips=False)"""
    from .dtu_metrics import evaluate_dtu_predictions
    scene, scan_id = scene_of(train_cfg, object_token)
    return evaluate_dtu_predictions(per_cam, scene, train_cfg.data.dtu_subset, train_cfg.data.dtu_lighting,
                                    train_cfg.data.dtu_preprocess_key, seeds, scan_id=scan_id,
                                    make_figures=make_figures, do_lpips=lpips_fn is not None, lpips_fn=lpips_fn)


def load_train_cfg(input_dir: Path, iteration: int):
    """the run's config from the view checkpoint's `cfg` (scripts/inference.py:63-66), extension keys included when the
    checkpoint carries them"""
    ckpt = torch.load(Path(input_dir) / f"mapper-steps-{iteration}_view.pt", map_location="cpu", weights_only=False)
    cfg = cfgmod.decode(cfgmod.RunConfig, CheckpointHandler.clean_config_dict(dict(ckpt["cfg"])))
    for k, v in ckpt.get("vneti_ext", {}).get("config_ext", {}).items():
        obj = cfg
        *path, name = k.split(".")
        for p in path:
            obj = getattr(obj, p)
        setattr(obj, name, v)
    if ckpt.get("vneti_ext", {}).get("synthetic_sd_weights"):
        cfg.model.allow_synthetic_weights = True
    return cfg


def run(icfg: InferenceConfig) -> Dict[Optional[str], dict]:
    """scripts/inference.py:60-135: every evaluation view x seed (x evaluation object in mode 3) -> one PNG per object
    and seed, and results_all_iter_*.pt"""
    from PIL import Image
    input_dir = Path(icfg.input_dir)
    train_cfg = load_train_cfg(input_dir, icfg.iteration)
    train_cfg.eval.num_denoising_steps = icfg.num_denoising_steps
    train_cfg.debug = icfg.debug
    train_cfg.log.exp_dir = input_dir
    if train_cfg.data.camera_representation != "dtu-12d":
        raise NotImplementedError("inference.py script only implemented for dtu dataset")
    if icfg.eval_placeholder_object_tokens:
        train_cfg.eval.eval_placeholder_object_tokens = list(icfg.eval_placeholder_object_tokens)
    pipe, pm = load_nvs_pipeline(train_cfg, icfg.iteration, icfg.batch, use_ema=icfg.use_ema)
    tokens = pipe.object_tokens
    if train_cfg.learnable_mode == 3:
        evals = list(train_cfg.eval.eval_placeholder_object_tokens or tokens[:1])
        for t in evals:
            if t not in tokens:
                raise ValueError(f"Item from eval_placeholder_object_tokens [{t}] not one of the training tokens, "
                                 f"which are {tokens}")
        objects = [eval_object_token(train_cfg, tokens, t) for t in evals]
        keys = evals
    else:
        # the reference raises NameError at :117 here (`results` is undefined outside mode 3); its evident intent,
        # results stored under the key None, is what is written
        objects, keys = [eval_object_token(train_cfg, tokens)], [None]
    from .dtu_metrics import get_cam_idxs
    cam_idxs, _, _ = get_cam_idxs(train_cfg.data.dtu_subset)
    seeds = list(icfg.seeds)
    pipe.timestep_spacing = icfg.timestep_spacing
    preds = generate_views(pipe, pm, objects, cam_idxs, seeds, icfg.num_denoising_steps,
                           guidance_rescale=icfg.guidance_rescale)
    out_dir = Path(icfg.inference_dir)
    out_dir.mkdir(parents=True, exist_ok=True)
    lpips_fn = None
    if icfg.do_lpips:
        from .lpips import LPIPS
        lpips_fn = LPIPS.from_files(icfg.lpips_vgg_weights, icfg.lpips_lin_weights)
    results = {}
    for key, obj in zip(keys, objects):
        res = evaluate(train_cfg, preds[obj], seeds, obj if train_cfg.learnable_mode == 3 else None, lpips_fn=lpips_fn)
        for i, grid in enumerate(res["grids"]):
            name = out_dir / preds_png_name(key, icfg.iteration, seeds[i])
            if res["figures"]:
                res["figures"][i].savefig(name, dpi=300)
            else:
                Image.fromarray((grid.clamp(0, 1).numpy() * 255).round().astype(np.uint8)).save(name)
        for k in ("figures", "grids", "imgs_gt_plot"):
            res.pop(k)
        results[key] = res
    torch.save(results, out_dir / results_name(icfg.iteration, list(results), seeds))
    return results
