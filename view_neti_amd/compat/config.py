"""Run configuration with the field names, defaults and `__post_init__` behaviour of the reference's
`training/config.py:11-293`, plus a small pyrallis-compatible front end (pyrallis is not installed on
either box): `--config_path file.yaml` + dotted `--a.b value` overrides, `encode`/`decode`/`dump`.

Deliberate deviation: the reference refuses `optim.train_batch_size > 3`
(config.py:269-271); the headline benchmark is bs=4, so the guard is a warning here.
"""
from __future__ import annotations

import dataclasses
import sys
import typing
import warnings
from dataclasses import dataclass, field, fields, is_dataclass
from pathlib import Path
from typing import Any, Dict, List, Optional, Union

import yaml

from .constants import VALIDATION_PROMPTS
from .pretrained_models import lookup_pretrained_models


@dataclass
class PESigmas:
    """utils/types.py:17-24 (the reference's `= float` default typo is not reproduced: defaults are None)."""
    sigma_t: float
    sigma_l: float
    sigma_theta: Optional[float] = None
    sigma_phi: Optional[float] = None
    sigma_r: Optional[float] = None
    sigma_dtu12: Optional[float] = None


@dataclass
class LogConfig:
    exp_name: str = ""
    overwrite_ok: bool = False
    exp_dir: Path = Path("./outputs")
    save_steps: int = 1000
    logging_dir: Path = Path("logs")
    report_to: str = "all"
    checkpoints_total_limit: Optional[int] = None
    save_dataset_images: bool = True
    # extensions (not in the reference, which saves mappers only and never finished its resume branch, coach.py:500-506):
    # `trainer-state-steps-N.pt` beside the mapper checkpoints of every `save_steps` — AdamW moments, step counts, loss
    # scale, device and host RNG streams, position in the shuffled epoch — from which `model.mapper_checkpoint_path` /
    # `auto_resume` continue bit-identically (compat/resume.py).  All off by default.  They are run control
    # ("run_control": True): they say how a process was launched, not what it trained, so a checkpoint's `vneti_ext` never
    # holds them, and config.yaml names them only where they are set — a run that does not use them writes the file it
    # always wrote
    save_trainer_state: bool = field(default=False, metadata={"ext": True, "run_control": True})
    # newest K states stay on disk (0 = all)
    keep_trainer_states: int = field(default=2, metadata={"ext": True, "run_control": True})
    # continue from the newest complete state in exp_dir
    auto_resume: bool = field(default=False, metadata={"ext": True, "run_control": True})
    # per-step training record (the reference logs total_loss and lr to its tracker after every micro-step,
    # coach.py:256-261): rank 0 appends one line per optimizer step to <exp_dir>/train-metrics.jsonl — loss, lr, loss
    # scale, skipped steps, gradient norms, clip coefficient and every sample's (timestep, loss) — produced on the device
    # inside the captured step and fetched where the loop already syncs (compat/train_metrics.py)
    train_metrics: bool = field(default=False, metadata={"ext": True, "run_control": True})


@dataclass
class DataConfig:
    train_data_dir: Path = None
    train_data_subsets: List[Path] = None
    placeholder_object_token: str = "<>"
    super_category_object_token: Optional[str] = "object"
    super_category_view_token: Optional[str] = "view"
    placeholder_object_tokens: List[str] = None
    super_category_object_tokens: Optional[List[str]] = None
    fixed_object_token_or_path: Union[str, Path] = None
    dataloader_num_workers: int = 8
    repeats: int = 100
    resolution: int = 512
    dtu_preprocess_key: int = 1
    center_crop: bool = False
    flip_p: float = 0.5
    caption_strategy: int = 0
    camera_representation: str = "spherical"
    dtu_lighting: str = 3
    dtu_subset: int = -2
    augmentation_key: int = 0
    # extension (not in the reference): run resize / flip / augmentations as HIP kernels on images cached in HBM
    # (engine/input_pipeline.py); same random draws, same pixels as the host path
    device_input_pipeline: bool = field(default=False, metadata={"ext": True})
    # extension (not in the reference): with augmentation_key 0 the dataset is deterministic (flip_p is never
    # forwarded, coach.py:682-702 vs dataset.py:52), so `vae.encode(pixels).latent_dist` (coach.py:165) — the MOMENTS, not the
    # sample — of an image is the same every time it comes up: keep them in HBM (64 KiB per 512^2 image) and re-draw only
    # `.sample()`.  Bit-identical training; the VAE encoder runs once per image instead of once per step.
    cache_vae_moments: bool = field(default=False, metadata={"ext": True})
    # extension: a folder of object masks; setting it weights the training loss per latent pixel by the
    # sample's mask (optim.loss_mask_background is the weight of the background).  DTU roots: the lookup of
    # dtu_metrics.get_object_masks, `<mask_dir>/scanN[/mask]/NNN.png` by camera index; any other root:
    # `<mask_dir>/<image stem>.png`.  A training image without a mask file is an error.  Same rules as optim.max_grad_norm:
    # it describes the trained model, named only where set
    mask_dir: Optional[Path] = field(default=None, metadata={"ext": True, "when_set": True})
    # filled at run time; a plain class attribute (NOT a dataclass field) as in the reference (config.py:64), so it
    # never enters config.yaml / the checkpoint's cfg dict
    placeholder_view_tokens = None

    def __post_init__(self):
        # annotated `str` with an int default in the reference (config.py:66); file-name matching needs str
        self.dtu_lighting = str(self.dtu_lighting)


_SIGMA_DTU12 = {1: 1.0, 2: 0.5, 3: 0.25, 4: 0.75, 5: 0.1}
_SIGMA_T = {0: 0.03, 1: 0.06, 2: 0.2, 3: 0.5}
_SIGMA_L = {0: 2.0, 1: 4.0}


@dataclass
class ModelConfig:
    pretrained_model_name_or_path: str = "CompVis/stable-diffusion-v1-4"
    pretrained_view_mapper: Path = None
    pretrained_view_mapper_key: int = None
    word_embedding_dim: int = 768
    arch_mlp_hidden_dims: int = 128
    use_nested_dropout: bool = True
    nested_dropout_prob: float = 0.5
    normalize_object_mapper_output: bool = True
    normalize_view_mapper_output: bool = False
    target_norm_object: float = None
    target_norm_view: float = None
    use_positional_encoding_object: int = 1
    use_positional_encoding_view: int = 1
    pe_sigmas: Any = field(default_factory=lambda: {"sigma_t": 0.03, "sigma_l": 2.0, "sigma_theta": 1.0,
                                                    "sigma_phi": 1.0, "sigma_r": 1.0, "sigma_dtu12": 2.0})
    pe_sigma_exp_key: int = 0
    pe_t_exp_key: int = 0
    pe_l_exp_key: int = 0
    pe_sigmas_view: Dict[str, float] = field(default_factory=lambda: {"sigma_phi": 1.0})
    num_pe_time_anchors: int = 10
    output_bypass_object: bool = True
    output_bypass_view: bool = True
    revision: Optional[str] = None
    mapper_checkpoint_path: Optional[Path] = None
    arch_view_net: int = 0
    arch_view_mix_streams: int = 0
    arch_view_disable_tl: bool = True
    original_ti: bool = False
    bypass_unconstrained_object: bool = False
    bypass_unconstrained_view: bool = False
    output_bypass_alpha_view: float = 0.2
    output_bypass_alpha_object: float = 0.2
    # extension: hub ids such as the reference default "CompVis/stable-diffusion-v1-4" cannot be resolved offline.
    # Training on SD-shaped SYNTHETIC weights must be asked for explicitly (benchmarks, tests); otherwise a
    # non-local `pretrained_model_name_or_path` is an error (compat/sd_weights.py)
    allow_synthetic_weights: bool = field(default=False, metadata={"ext": True})

    def __post_init__(self):
        # config.py:142-178 — the YAML sigma values are overridden by the *_exp_key switches (App. C Q3)
        if self.pe_sigmas is None:
            return
        src = dataclasses.asdict(self.pe_sigmas) if isinstance(self.pe_sigmas, PESigmas) else dict(self.pe_sigmas)
        phi = src.get("sigma_phi", 1.0)
        phi = 1.0 if phi is None else phi
        dtu = src.get("sigma_dtu12", 2.0)
        sig = PESigmas(sigma_t=src["sigma_t"], sigma_l=src["sigma_l"], sigma_theta=phi, sigma_phi=phi, sigma_r=phi,
                       sigma_dtu12=2.0 if dtu is None else dtu)
        if self.pe_sigma_exp_key in _SIGMA_DTU12:
            sig.sigma_dtu12 = _SIGMA_DTU12[self.pe_sigma_exp_key]
        if self.pe_t_exp_key not in _SIGMA_T:
            raise ValueError(f"unknown pe_t_exp_key {self.pe_t_exp_key}")
        sig.sigma_t = _SIGMA_T[self.pe_t_exp_key]
        if self.pe_l_exp_key not in _SIGMA_L:
            raise ValueError(f"unknown pe_l_exp_key {self.pe_l_exp_key}")
        sig.sigma_l = _SIGMA_L[self.pe_l_exp_key]
        self.pe_sigmas = sig


@dataclass
class EvalConfig:
    validation_prompts: List[str] = field(default_factory=lambda: list(VALIDATION_PROMPTS))
    num_validation_images: int = 3
    validation_seeds: Optional[List[int]] = field(default_factory=lambda: [0, 1, 2])
    validation_steps: int = 250
    num_denoising_steps: int = 30
    dtu_upsample_key: int = 1
    eval_placeholder_object_tokens: List[str] = None
    # extensions (not in the reference), all off by default and run control like log.save_trainer_state: they
    # say how a run is watched, not what it trained.
    # held-out diffusion loss (compat/heldout.py): every N optimizer steps and at the last one, the forward half of the
    # train step on the 34 DTU evaluation views at K fixed timesteps t_k = floor((2k+1) T / (2K)) with fixed noise
    # (generator seed = heldout_loss_seed + 1000 * camera + k), split into train / test cameras -> heldout-loss.jsonl
    heldout_loss_steps: int = field(default=0, metadata={"ext": True, "run_control": True})
    heldout_loss_timesteps: int = field(default=4, metadata={"ext": True, "run_control": True})
    heldout_loss_seed: int = field(default=0, metadata={"ext": True, "run_control": True})
    # the reference's validation (training/validate.py:65-186): render the 34 evaluation views x validation_seeds at the
    # novel-view resolution, `validation_nvs_batch` prompts per sampler run, and score them against the scene
    validation_nvs: bool = field(default=False, metadata={"ext": True, "run_control": True})
    validation_nvs_batch: int = field(default=4, metadata={"ext": True, "run_control": True})
    # LPIPS(net="vgg") for that scoring (compat/lpips.py; fp16 runs only): torchvision's vgg16 and lpips' linear heads
    lpips_vgg_weights: Optional[Path] = field(default=None, metadata={"ext": True, "run_control": True})
    lpips_lin_weights: Optional[Path] = field(default=None, metadata={"ext": True, "run_control": True})
    # run the validation (images, and validation_nvs) on the EMA of the mappers (optim.ema_decay)
    validation_use_ema: bool = field(default=False, metadata={"ext": True, "run_control": True})
    # the validation renders' sampler (Lin et al. 2023, for v-prediction models): diffusers' guidance_rescale in
    # [0, 1] and the schedulers' timestep_spacing (None | "trailing").  They touch no training step.
    guidance_rescale: float = field(default=0.0, metadata={"ext": True, "run_control": True})
    timestep_spacing: Optional[str] = field(default=None, metadata={"ext": True, "run_control": True})
    # a "loss_masked" value beside every held-out loss: the same residual under the evaluation view's object mask at the
    # training resolution.  Needs data.mask_dir
    heldout_loss_masked: bool = field(default=False, metadata={"ext": True, "run_control": True})
    # plain class attribute in the reference too (config.py:188)
    validation_view_tokens = None

    def __post_init__(self):
        if self.validation_seeds is None:
            self.validation_seeds = list(range(self.num_validation_images))
        assert len(self.validation_seeds) == self.num_validation_images, \
            "Length of validation_seeds should equal num_validation_images"
        if self.heldout_loss_steps < 0 or self.heldout_loss_timesteps < 1 or self.validation_nvs_batch < 1:
            raise ValueError("eval: heldout_loss_steps >= 0, heldout_loss_timesteps >= 1 and validation_nvs_batch >= 1")
        if not 0.0 <= self.guidance_rescale <= 1.0:
            raise ValueError(f"eval.guidance_rescale = {self.guidance_rescale}: it lies in [0, 1] (0: off)")
        if self.timestep_spacing not in (None, "trailing"):
            raise ValueError(f"eval.timestep_spacing {self.timestep_spacing!r}: None (the scheduler's default) or 'trailing'")


@dataclass
class OptimConfig:
    max_train_steps: Optional[int] = 1_000
    learning_rate: float = 1e-3
    scale_lr: bool = True
    train_batch_size: int = 3
    gradient_checkpointing: bool = False
    gradient_accumulation_steps: int = 3
    seed: Optional[int] = None
    lr_scheduler: str = "constant"
    lr_warmup_steps: int = 0
    adam_beta1: float = 0.9
    adam_beta2: float = 0.999
    adam_weight_decay: float = 1e-2
    adam_epsilon: float = 1e-08
    mixed_precision: str = "no"
    allow_tf32: bool = False
    # extension: clip the mappers' global gradient norm before AdamW, accelerator.clip_grad_norm_ /
    # torch.nn.utils.clip_grad_norm_ semantics.  It describes the trained model (not run control): it travels beside a
    # checkpoint's cfg and enters the resume fingerprint — where it is set ("when_set": config.yaml and a checkpoint's
    # extension fields of a run without it are the ones they always were)
    max_grad_norm: Optional[float] = field(default=None, metadata={"ext": True, "when_set": True})
    # extensions, the two objective controls of diffusers' trainers, under the same rules as max_grad_norm:
    # snr_gamma — Min-SNR-gamma loss weighting (--snr_gamma; `inf` weights every timestep alike); noise_offset — offset
    # noise, noise += noise_offset * randn(B, C, 1, 1) (--noise_offset).  Held-out losses stay unweighted and offset-free.
    snr_gamma: Optional[float] = field(default=None, metadata={"ext": True, "when_set": True})
    noise_offset: Optional[float] = field(default=None, metadata={"ext": True, "when_set": True})
    # extension: an exponential moving average of the mappers, kept on the device inside the captured step
    # (diffusers' --use_ema / EMAModel with inv_gamma 1, min_decay 0).  ema_decay is the cap of the decay, in (0, 1);
    # ema_update_after_step delays the averaging; ema_warmup_power None is the (1 + s) / (10 + s) ramp, a value > 0 the
    # 1 - (1 + s)^(-power) one.  Same rules as max_grad_norm: they describe the trained model, named only where set
    ema_decay: Optional[float] = field(default=None, metadata={"ext": True, "when_set": True})
    ema_update_after_step: int = field(default=0, metadata={"ext": True, "when_set": True})
    ema_warmup_power: Optional[float] = field(default=None, metadata={"ext": True, "when_set": True})
    # extension: the weight of a background pixel in the object-masked loss that data.mask_dir turns on, in
    # [0, 1] (0: the background carries no gradient; 1: the plain loss).  Same rules as max_grad_norm
    loss_mask_background: float = field(default=0.0, metadata={"ext": True, "when_set": True})

    def __post_init__(self):
        if not 0.0 <= self.loss_mask_background <= 1.0:
            raise ValueError(f"optim.loss_mask_background must lie in [0, 1] (is {self.loss_mask_background})")
        if self.ema_decay is not None and not 0.0 < self.ema_decay < 1.0:
            raise ValueError(f"optim.ema_decay must be in (0, 1) when set (is {self.ema_decay})")
        if self.ema_warmup_power is not None and not 0.0 < self.ema_warmup_power < float("inf"):
            raise ValueError(f"optim.ema_warmup_power must be > 0 and finite when set (is {self.ema_warmup_power})")
        if self.ema_update_after_step < 0:
            raise ValueError(f"optim.ema_update_after_step must be >= 0 (is {self.ema_update_after_step})")
        if self.ema_decay is None and (self.ema_update_after_step or self.ema_warmup_power is not None):
            raise ValueError("optim.ema_update_after_step / optim.ema_warmup_power need optim.ema_decay")
        for name in ("max_grad_norm", "snr_gamma", "noise_offset"):
            v = getattr(self, name)
            if v is not None and not v > 0:
                raise ValueError(f"optim.{name} must be > 0 when set (is {v})")
        if self.noise_offset is not None and self.noise_offset == float("inf"):
            raise ValueError("optim.noise_offset must be finite")


@dataclass
class RunConfig:
    learnable_mode: int = 0
    debug: bool = False
    seed: int = 0
    log: LogConfig = field(default_factory=LogConfig)
    data: DataConfig = field(default_factory=DataConfig)
    model: ModelConfig = field(default_factory=ModelConfig)
    eval: EvalConfig = field(default_factory=EvalConfig)
    optim: OptimConfig = field(default_factory=OptimConfig)

    def __post_init__(self):
        if self.optim.train_batch_size > 3:
            warnings.warn("reference config.py:269-271 rejects train_batch_size > 3; allowed here (bench uses bs=4)")
        if self.learnable_mode == 3:
            assert self.data.dataloader_num_workers == 0, "can't support multiple workers right now for learnable mode 3"
            assert self.data.super_category_object_tokens is not None
            if self.eval.eval_placeholder_object_tokens is not None:
                assert all(d in self.data.placeholder_object_tokens for d in self.eval.eval_placeholder_object_tokens), \
                    "eval.eval_placeholder_tokens not in data.placeholder_object_tokens"
        if self.data.placeholder_object_tokens is not None:
            assert len(self.data.placeholder_object_tokens) == len(set(self.data.placeholder_object_tokens)), \
                "cfg.data.placeholder_object_tokens must be unique strings"
        if self.optim.loss_mask_background != 0.0 and self.data.mask_dir is None:
            raise ValueError("optim.loss_mask_background needs data.mask_dir")
        if self.eval.heldout_loss_masked and self.data.mask_dir is None:
            raise ValueError("eval.heldout_loss_masked needs data.mask_dir")
        if self.learnable_mode in (4, 5):
            assert self.model.pretrained_view_mapper or self.model.pretrained_view_mapper_key
            if self.model.pretrained_view_mapper_key:
                self.model.pretrained_view_mapper = lookup_pretrained_models[str(self.model.pretrained_view_mapper_key)]


# ----------------------------------------------------------------------------------------------
# mini-pyrallis
# ----------------------------------------------------------------------------------------------
def encode(obj, include_ext: bool = True):
    """pyrallis.encode: dataclass -> plain dict (Path -> str), used for config.yaml and inside checkpoints
    (training/logger.py:25-28, checkpoint_handler.py:59,64).  `include_ext=False` leaves out the fields this repo
    adds to the reference's schema (metadata ext=True): the reference's `pyrallis.decode(RunConfig, ckpt['cfg'])`
    (checkpoint_handler.py:142) rejects keys it does not know.  Run-control extensions appear only where they are set."""
    if is_dataclass(obj) and not isinstance(obj, type):
        return {f.name: encode(getattr(obj, f.name), include_ext) for f in fields(obj)
                if (include_ext or not f.metadata.get("ext"))
                and not ((f.metadata.get("run_control") or f.metadata.get("when_set")) and getattr(obj, f.name) == f.default)}
    if isinstance(obj, Path):
        return str(obj)
    if isinstance(obj, dict):
        return {k: encode(v, include_ext) for k, v in obj.items()}
    if isinstance(obj, (list, tuple)):
        return [encode(v, include_ext) for v in obj]
    return obj


def ext_fields(obj) -> Dict[str, Any]:
    """{"section.field": value} of the extension fields that describe the trained model or its data (stored beside, not
    inside, a checkpoint's cfg); run-control extensions (metadata "run_control") stay out of checkpoints."""
    out = {}
    for f in fields(obj):
        v = getattr(obj, f.name)
        if is_dataclass(v):
            out.update({f"{f.name}.{k}": x for k, x in ext_fields(v).items()})
        elif f.metadata.get("ext") and not f.metadata.get("run_control") \
                and not (f.metadata.get("when_set") and v == f.default):
            out[f.name] = v
    return out


def _coerce(tp, val):
    if val is None:
        return None
    origin = typing.get_origin(tp)
    if origin is Union:
        args = [a for a in typing.get_args(tp) if a is not type(None)]
        for a in args:
            try:
                return _coerce(a, val)
            except (TypeError, ValueError):
                continue
        return val
    if origin in (list, List):
        (a,) = typing.get_args(tp) or (Any,)
        if isinstance(val, str):
            val = yaml.safe_load(val)
        return [_coerce(a, v) for v in val]
    if origin in (dict, Dict):
        return yaml.safe_load(val) if isinstance(val, str) else dict(val)
    if tp is Path:
        return Path(val)
    if tp is bool:
        return val if isinstance(val, bool) else str(val).lower() in ("1", "true", "yes")
    if tp in (int, float, str):
        return tp(val)
    if isinstance(tp, type) and is_dataclass(tp):
        return decode(tp, val)
    if isinstance(val, str) and tp is Any:
        try:
            return yaml.safe_load(val)
        except yaml.YAMLError:
            return val
    return val


def decode(cls, d: Dict[str, Any]):
    """pyrallis.decode: plain dict -> dataclass (checkpoint_handler.py:142).  Unknown keys are an error, as with
    pyrallis (a typo in a YAML file or a dotted override must not be dropped silently)."""
    hints = typing.get_type_hints(cls)
    names = {f.name for f in fields(cls)}
    unknown = sorted(set(d) - names)
    if unknown:
        raise ValueError(f"{cls.__name__}: unknown configuration key(s) {unknown}")
    kwargs = {}
    for f in fields(cls):
        if f.name in d:
            kwargs[f.name] = _coerce(hints[f.name], d[f.name])
    return cls(**kwargs)


def dump(cfg, stream=None) -> Optional[str]:
    text = yaml.safe_dump(encode(cfg), sort_keys=False)
    if stream is None:
        return text
    stream.write(text)
    return None


def _set_dotted(d: Dict[str, Any], key: str, value):
    parts = key.split(".")
    for p in parts[:-1]:
        d = d.setdefault(p, {})
    d[parts[-1]] = value


def parse(cls=RunConfig, args: Optional[List[str]] = None):
    """`--config_path file.yaml` first, then dotted overrides `--optim.train_batch_size 4`
    (README.md:40-44 of the reference); a bare flag such as `--log.overwrite_ok` means True."""
    args = list(sys.argv[1:] if args is None else args)
    d: Dict[str, Any] = {}
    overrides = []
    i = 0
    while i < len(args):
        a = args[i]
        if not a.startswith("--"):
            raise SystemExit(f"unexpected argument {a!r}")
        key = a[2:]
        if "=" in key:
            key, val = key.split("=", 1)
            i += 1
        elif i + 1 < len(args) and not args[i + 1].startswith("--"):
            val = args[i + 1]
            i += 2
        else:
            val = True
            i += 1
        if key == "config_path":
            with open(val) as f:
                d = yaml.safe_load(f) or {}
        else:
            overrides.append((key, val))
    for key, val in overrides:
        _set_dotted(d, key, val)
    return decode(cls, d)


def wrap():
    """decorator with pyrallis.wrap()'s calling convention (scripts/train.py:19)."""
    def deco(fn):
        def inner(*a, **k):
            hints = typing.get_type_hints(fn)
            cls = next(iter(hints.values()))
            return fn(parse(cls), *a, **k)
        return inner
    return deco
