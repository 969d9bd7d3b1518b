"""Generation from a finished training run — the role of the reference's `training/inference_dtu.py:283-398`
(`load_stable_diffusion_model`, mapper loading through `CheckpointHandler.load_mapper`, `PromptManager`,
`sd_pipeline_call`) without its DTU evaluation harness (SURVEY §8 f4 stays out of scope).

    pipe, pm = load_inference(exp_dir, "mapper-final", batch=1)       # config.yaml + mapper-final_{object,view}.pt
    out = sd_pipeline_call(pipe, pm.embed_prompt("<view_…>. A photo of a <object>"), num_inference_steps=30,
                           generator=torch.Generator().manual_seed(0))
    out.images[0].save("img.png")

The tokenizer is rebuilt exactly like `Coach` does it (view tokens first, then object tokens: the token ids the
mappers were trained with), the frozen SD weights come from `model.pretrained_model_name_or_path` (a local
diffusers directory) or the synthetic generator, and the new embedding rows are initialised from the
super-category rows — they are never read, the mappers overwrite them, but the table must have the rows.
"""
from __future__ import annotations

from pathlib import Path
from typing import Optional, Tuple

import torch
import yaml

from .. import sd_config as sc
from ..engine.infer import InferenceEngine
from ..engine.text import flatten_mapper_state
from . import config as cfgmod
from .checkpoint_handler import CheckpointHandler
from .coach import _sd_family
from .dataset import TextualInversionDataset
from .neti_modules import NeTIMapper
from .prompt_manager import PromptManager
from .sd_pipeline_call import InferencePipeline
from .sd_weights import load_sd_weights, load_vae_decoder_weights
from .tokenizer import load_tokenizer


def load_inference(exp_dir, mapper_stem: str = "mapper-final", batch: int = 1, height: Optional[int] = None,
                   width: Optional[int] = None, object_token: Optional[str] = None, sampler: str = "dpm++2m",
                   device: str = "cuda", per_sample: bool = False) -> Tuple[InferencePipeline, PromptManager]:
    """per_sample: all object mappers of the run go into one bucket and every sample of a batch picks its own
    (`sd_pipeline_call` with a list of PromptEmbeds); otherwise the engine holds `object_token`'s mapper only."""
    exp_dir = Path(exp_dir)
    with (exp_dir / "config.yaml").open() as f:
        cfg = cfgmod.decode(cfgmod.RunConfig, CheckpointHandler.clean_config_dict(yaml.safe_load(f)))
    return build_inference(cfg, exp_dir, mapper_stem, batch, height, width, object_token, sampler, device, per_sample)


def build_inference(cfg, exp_dir, mapper_stem: str, batch: int = 1, height: Optional[int] = None,
                    width: Optional[int] = None, object_token: Optional[str] = None, sampler: str = "dpm++2m",
                    device: str = "cuda", per_sample: bool = False, view_stem: Optional[str] = None
                    ) -> Tuple[InferencePipeline, PromptManager]:
    """load_inference with the run's config given (the reference's evaluation reads it from the view checkpoint).
    view_stem: the view mapper's file stem where it differs from the object mapper's (averaged object mapper beside a frozen
    view mapper)"""
    exp_dir = Path(exp_dir)
    sd = _sd_family(cfg)
    tok = load_tokenizer(str(cfg.model.pretrained_model_name_or_path), sd.clip.vocab_size)
    obj_path, view_path = exp_dir / f"{mapper_stem}_object.pt", exp_dir / f"{view_stem or mapper_stem}_view.pt"
    if obj_path.exists():
        raw = torch.load(obj_path, map_location="cpu", weights_only=False)
        object_tokens = [e["placeholder_object_token"] for e in raw["mappers"].values()]
    elif per_sample and cfg.learnable_mode == 1:
        object_tokens = []  # mode 1 trains no object mapper: the prompts hold the fixed word (dataset.py:654-668)
    else:
        raise FileNotFoundError(obj_path)
    view_tokens = []
    cam_fn = None
    mapper_view = None
    if view_path.exists():
        lut_tok, lut_par = TextualInversionDataset.dtu_generate_dset_cam_tokens_params()
        view_tokens = [lut_tok[k] for k in sorted(lut_tok)]
    tok.add_tokens(view_tokens + object_tokens)
    view_ids = tok.convert_tokens_to_ids(view_tokens) if view_tokens else []
    object_ids = tok.convert_tokens_to_ids(object_tokens) if object_tokens else []
    lookup = {}
    if object_tokens:
        _, lookup = CheckpointHandler.load_mapper(obj_path, "object", object_tokens, object_ids)
    if view_path.exists():
        cams = torch.stack([lut_par[k] for k in sorted(lut_par)])
        mins, maxs = cams.min(0).values.flatten(), cams.max(0).values.flatten()
        _, mapper_view = CheckpointHandler.load_mapper(view_path, "view", cam_mins=mins, cam_maxs=maxs)
        id2tok = dict(zip(view_ids, view_tokens))

        def cam_fn(token_id: int) -> torch.Tensor:
            p = TextualInversionDataset.dtu_token_to_cam_params(id2tok[token_id])[0]
            return (p - mins) / (maxs - mins) * 2 - 1
    if object_tokens:
        object_token = object_token or object_tokens[0]
        mo = lookup[tok.convert_tokens_to_ids(object_token)]
    else:  # a stand-in that no prompt reaches (placeholder -1 on every row)
        mo = NeTIMapper(embedding_type="object", output_dim=cfg.model.word_embedding_dim,
                        arch_mlp_hidden_dims=cfg.model.arch_mlp_hidden_dims, norm_scale=None,
                        pe_sigmas=cfg.model.pe_sigmas, arch_view_net=cfg.model.arch_view_net,
                        num_pe_time_anchors=cfg.model.num_pe_time_anchors)
    allow = cfg.model.allow_synthetic_weights
    unet_w, _, clip_w, synthetic = load_sd_weights(sd, str(cfg.model.pretrained_model_name_or_path), device, allow)
    dec_w, _ = load_vae_decoder_weights(sd, str(cfg.model.pretrained_model_name_or_path), device, allow)
    # grow the token table like Coach._extend_token_embedding (rows are placeholders for the mapper outputs)
    key = "text_model.embeddings.token_embedding.weight"
    E = clip_w[key]
    extra = len(tok) - E.shape[0]
    if extra > 0:
        so = tok.encode(cfg.data.super_category_object_token, add_special_tokens=False)[0]
        clip_w = dict(clip_w)
        clip_w[key] = torch.cat([E, E[so].unsqueeze(0).repeat(extra, 1)], 0)
    if height is None or width is None:
        if "dtu" in str(cfg.data.train_data_dir) and cfg.learnable_mode != 0:
            height, width = {0: (512, 512), 1: (384, 512), 2: (576, 768)}[cfg.data.dtu_preprocess_key]
        else:
            height = width = cfg.data.resolution
    m = cfg.model
    kw = {}
    if mapper_view is not None:
        kw = dict(mapper_view=mapper_view.mapper_state(), w_enc_view=mapper_view.encoder.w,
                  norm_scale_view=mapper_view.norm_scale, alpha_view=m.output_bypass_alpha_view,
                  unconstrained_view=m.bypass_unconstrained_view, output_bypass_view=mapper_view.output_bypass)
    object_slot = None
    if per_sample:
        # every object mapper of the run in one bucket, 4-float aligned slots (the 16-byte weight loads of each slot)
        mappers = [lookup[i] for i in object_ids] or [mo]
        if any(not torch.equal(x.encoder.w, mappers[0].encoder.w) for x in mappers):
            # the engine holds one encoder table for the bucket (the legacy mapper's frequencies are drawn per object)
            raise NotImplementedError("per-sample object slots need one encoder-frequency table shared by all objects")
        flats = [flatten_mapper_state(x.mapper_state()) for x in mappers]
        stride = (flats[0].numel() + 3) // 4 * 4
        bucket = torch.zeros(stride * len(flats))
        for k, f in enumerate(flats):
            bucket[k * stride:k * stride + f.numel()] = f
        kw.update(params_object=bucket.to(device), object_slot_stride=stride, per_sample_slots=True)
        object_slot = {tid: k for k, tid in enumerate(object_ids)}
    eng = InferenceEngine(sd, unet_w, dec_w, clip_w, batch, height, width, mo.mapper_state(), mo.encoder.w,
                          mo.norm_scale, m.output_bypass_alpha_object, hidden_object=mo.hidden,
                          unconstrained_object=m.bypass_unconstrained_object, device=device,
                          **mo.engine_encoder_kwargs(), **kw)
    pipe = InferencePipeline(eng, tok, sampler, object_slot=object_slot)
    pm = PromptManager(tok, placeholder_view_token_ids=view_ids, placeholder_object_token_ids=object_ids,
                       view_params_fn=cam_fn)
    pipe.synthetic_weights = synthetic
    pipe.object_tokens = object_tokens
    pipe.cfg = cfg
    return pipe, pm
