"""`sd_pipeline_call` with the argument surface of the reference's sd_pipeline_call.py:8-133, running on
`view_neti_amd.engine.infer.InferenceEngine` instead of a diffusers `StableDiffusionPipeline`.

    pipeline        -> an `InferencePipeline` (engine + tokenizer; built once per resolution/batch)
    prompt_embeds   -> EITHER the reference's own contract (sd_pipeline_call.py:86-92): a list of T per-step XTI dicts
                       (what the reference's PromptManager.embed_prompt returns, prompt_manager.py:79-99), one dict, or one
                       (B, 77, D) tensor — fed straight to the UNet's per-layer K / V sources, the engine's text pass skipped;
                       OR the light `PromptEmbeds` record of this package's PromptManager (conditioning computed inside
                       the loop, 16 layers per launch schedule), OR a list of B such records: one prompt per sample of the
                       batch (different views / objects; an engine built with per_sample_slots maps each sample's object
                       token to its mapper through `pipeline.object_slot`)
    generator       -> one torch.Generator, or a list of B (diffusers' prepare_latents): sample i is then
                       randn((1, 4, h, w), generator[i]), the draw a B = 1 call with that generator makes
    height / width  -> fixed at engine construction; passing different values raises
    scheduler       -> `pipeline.sampler` ("dpm++2m" as installed by validate.py:568, or "ddim")
    eta             -> DDIMScheduler.step's eta (prepare_extra_step_kwargs, sd_pipeline_call.py:66,101); eta > 0 draws one
                       randn((B, 4, h, w)) per sampler step from `generator`, after the initial latents and in step order
                       (a list of B generators: (1, 4, h, w) each from its own), as the scheduler's `variance_noise`;
                       with "dpm++2m" a non-zero eta raises (that scheduler has no eta; the reference drops it silently)
    guidance_rescale -> not in the reference's signature: diffusers' StableDiffusionPipeline.__call__ argument of that name
                       (Lin et al. 2023, `rescale_noise_cfg`), in [0, 1]; 0 (the default) is the reference's loop
    timestep_spacing -> `pipeline.timestep_spacing`, a scheduler property like the sampler: None or "trailing"
Returns an object with `.images` (list of PIL images, `output_type="pil"`) or the array, like the reference.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Any, Dict, List, Optional, Union

import numpy as np
import torch

from ..engine.infer import InferenceEngine, check_eta, check_rescale
from .prompt_manager import PromptEmbeds


@dataclass
class InferencePipeline:
    engine: InferenceEngine
    tokenizer: Any
    sampler: str = "dpm++2m"
    object_slot: Optional[Dict[int, int]] = None  # object token id -> mapper slot of the engine's bucket (per-sample prompts)
    timestep_spacing: Optional[str] = None  # the scheduler's timestep_spacing: None (its default list) or "trailing"


@dataclass
class PipelineOutput:
    images: Any
    nsfw_content_detected: Optional[bool] = False


def get_neg_prompt_input_ids(pipeline: InferencePipeline, negative_prompt: Optional[Union[str, List[str]]] = None):
    """sd_pipeline_call.py:136-150: tokenizer(negative_prompt or "", padding="max_length", truncation=True)."""
    if negative_prompt is None:
        negative_prompt = ""
    toks = [negative_prompt] if isinstance(negative_prompt, str) else negative_prompt
    return pipeline.tokenizer(toks, padding="max_length", max_length=pipeline.tokenizer.model_max_length,
                              truncation=True, return_tensors="pt")


def set_prompt_list(pipeline: InferencePipeline, prompts: List[PromptEmbeds]) -> None:
    """B PromptEmbeds -> InferenceEngine.set_prompts (ids, placeholders, camera parameters, object slot per sample)"""
    eng = pipeline.engine
    if len(prompts) != eng.B:
        raise ValueError(f"{len(prompts)} prompts for an engine built for batch {eng.B}")
    ids = torch.cat([p.input_ids.reshape(1, -1) for p in prompts])
    po = torch.cat([p.input_ids_placeholder_object.reshape(1) for p in prompts])
    pv = torch.cat([p.input_ids_placeholder_view.reshape(1) for p in prompts])
    with_view = [p.view_params is not None for p in prompts]
    vp = torch.cat([p.view_params.reshape(1, -1) for p in prompts]) if all(with_view) else None
    if any(with_view) and vp is None:
        raise ValueError("either every prompt of the batch holds a view token or none does")
    slots = None
    if eng.slots is not None:
        table = pipeline.object_slot or {}
        slots = [table.get(int(t), 0) for t in po]
    eng.set_prompts(ids, po, pv, vp, slots, [p.truncation_idx for p in prompts])


def _randn(eng: InferenceEngine, generator) -> torch.Tensor:
    """diffusers' randn_tensor for a latent-shaped draw: one generator draws the whole batch, a list of B draws
    (1, 4, h, w) each, so that sample i depends on generator[i] alone"""
    if isinstance(generator, list):
        if len(generator) != eng.B:
            raise ValueError(f"{len(generator)} generators for a batch of {eng.B}")
        return torch.cat([torch.randn((1, eng.Lc, eng.h, eng.w), generator=g, dtype=torch.float32) for g in generator])
    return torch.randn((eng.B, eng.Lc, eng.h, eng.w), generator=generator, dtype=torch.float32)


@torch.no_grad()
def sd_pipeline_call(pipeline: InferencePipeline, prompt_embeds: Union[PromptEmbeds, List[Dict[str, Any]], Dict[str, Any],
                                                                       torch.Tensor], height: Optional[int] = None,
                     width: Optional[int] = None, num_inference_steps: int = 50, guidance_scale: float = 7.5,
                     negative_prompt: Optional[Union[str, List[str]]] = None, num_images_per_prompt: Optional[int] = 1,
                     eta: float = 0.0, generator: Optional[Union[torch.Generator, List[torch.Generator]]] = None,
                     latents: Optional[torch.Tensor] = None, output_type: Optional[str] = "pil",
                     return_dict: bool = True, guidance_rescale: float = 0.0):
    eng = pipeline.engine
    B = eng.B
    H, W = eng.h * 8, eng.w * 8
    if (height or H) != H or (width or W) != W:
        raise ValueError(f"the engine was built for {H}x{W}")
    if num_images_per_prompt != B:
        raise ValueError(f"the engine was built for {B} images per call (num_images_per_prompt={num_images_per_prompt})")
    noisy = check_eta(pipeline.sampler, eta)  # eta != 0 on a sampler without one: ValueError, before any draw
    check_rescale(guidance_rescale)  # outside [0, 1]: ValueError, before any draw
    neg = get_neg_prompt_input_ids(pipeline, negative_prompt)
    eng.set_negative_prompt(neg.input_ids)
    if latents is None:  # pipeline.prepare_latents: randn(shape, generator) * init_noise_sigma (= 1)
        latents = _randn(eng, generator)
    # DDIMScheduler.step draws its variance noise inside the loop, after prepare_latents: one draw per step, in step order
    extra = dict(eta=eta, step_noise=torch.stack([_randn(eng, generator) for _ in range(num_inference_steps)])) \
        if noisy else {}
    if guidance_rescale:
        extra["guidance_rescale"] = guidance_rescale
    if pipeline.timestep_spacing is not None:
        extra["timestep_spacing"] = pipeline.timestep_spacing
    if isinstance(prompt_embeds, list) and prompt_embeds and all(isinstance(p, PromptEmbeds) for p in prompt_embeds):
        # one prompt per sample (distinct from the reference's list of per-step dicts: dispatch on the element type)
        set_prompt_list(pipeline, prompt_embeds)
        out = eng.generate(latents.to(eng.dev), num_inference_steps, guidance_scale, pipeline.sampler,
                           decode=output_type != "latent", **extra)
    elif isinstance(prompt_embeds, PromptEmbeds):
        rep = lambda t: None if t is None else t.expand(B, *t.shape[1:]) if t.dim() > 1 else t.expand(B)
        eng.set_prompt(rep(prompt_embeds.input_ids), rep(prompt_embeds.input_ids_placeholder_object),
                       rep(prompt_embeds.input_ids_placeholder_view), rep(prompt_embeds.view_params),
                       prompt_embeds.truncation_idx)
        out = eng.generate(latents.to(eng.dev), num_inference_steps, guidance_scale, pipeline.sampler,
                           decode=output_type != "latent", **extra)
    elif isinstance(prompt_embeds, (list, dict, torch.Tensor)):
        # the reference's contract: conditioning computed by the caller, `prompt_embeds[i]` per step when a list (:86)
        out = eng.generate_from_contexts(latents.to(eng.dev), prompt_embeds, num_inference_steps, guidance_scale,
                                         pipeline.sampler, decode=output_type != "latent", **extra)
    else:
        raise TypeError(f"prompt_embeds of type {type(prompt_embeds).__name__}: expected PromptEmbeds, a list of per-step "
                        "context dicts, one dict or one tensor")
    if output_type == "latent":
        image, nsfw = out.clone(), None
    else:
        image = out.cpu().numpy()  # (B, H, W, 3) f32 in [0,1] = decode_latents' output
        nsfw = False
        if output_type == "pil":
            from PIL import Image
            image = [Image.fromarray(im) for im in (image * 255).round().astype(np.uint8)]
    if not return_dict:
        return image, nsfw
    return PipelineOutput(images=image, nsfw_content_detected=nsfw)
