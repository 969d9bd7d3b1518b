"""Inference with learned NeTI mappers on the HIP engines: the loop of the reference's
`sd_pipeline_call` (sd_pipeline_call.py:8-133) with `PromptManager.embed_prompt`'s per-timestep, per-layer
text conditioning (prompt_manager.py:43-101) computed inside the loop.

Per denoising step i (timestep t_i):
    contexts   = 16 x [NeTI mapper(t_i, layer) -> CLIP -> bypass -> final LN]      TextEngine.forward (one batched pass)
    [eps_u; eps_c] = UNet([x; x], t_i, [uncond ctx; NeTI ctx])                      one CFG-batched UNetEngine.forward
    x <- sampler(x, eps_u + g (eps_c - eps_u))                                      vneti_cfg_sampler_step
then  image = (decode(x / scaling)/2 + 0.5).clamp(0,1)                              VAEDecoderEngine.forward

What differs from the reference on purpose: the two UNet calls of a step run as one batch of 2B (the reference
runs them back to back, :78-94); the T x 16 text-encoder passes are not materialised up front (the reference
holds T dicts of 32 tensors) but produced per step, 16 layers at a time; the unconditional embedding is computed
once.  Samplers: DPM-Solver++(2M) (the scheduler validate.py:568 / inference_dtu.py:304 install) and DDIM,
both as x <- cx x + c0 x0 + c1 x0_prev on the data prediction; DDIM with eta > 0 adds cn * noise, the noise of each step
read from a device table so that the step still replays as one graph (vneti_cfg_sampler_step_noise_table).
Guidance rescale (Lin et al. 2023; diffusers' `guidance_rescale`) multiplies the guided prediction of sample b by
f[b] = phi std(cond[b]) / std(guided[b]) + 1 - phi before the step: vneti_cfg_rescale_factor (two launches) and the
scaled step entries replace the step launch, in the eager loop and inside the captured step alike.
"""
from __future__ import annotations

from functools import partial
from typing import Dict, List, Optional, Sequence

import torch

from .. import lib, ops
from .. import sd_config as sc
from .graphs import capture_graphs
from .step import alphas_cumprod
from .text import MapperState, TextEngine, flatten_mapper_state
from .unet import UNetEngine
from .vae import VAEDecoderEngine


def inference_timesteps(kind: str, num_steps: int, num_train: int = 1000, spacing: Optional[str] = None) -> List[int]:
    """DPMSolverMultistepScheduler.set_timesteps: linspace(0, T-1, N+1).round()[::-1][:-1];
    DDIMScheduler.set_timesteps with steps_offset=1 (the SD scheduler configs): arange(N)*(T//N) reversed + 1.
    spacing="trailing" (both schedulers' timestep_spacing; Lin et al. 2023, "sample from the last timestep"):
    round(arange(T, 0, -T/N)) - 1, which starts at T - 1; None keeps the lists above."""
    import numpy as np
    if kind not in ("dpm++2m", "ddim"):
        raise ValueError(f"unknown sampler {kind!r} (dpm++2m | ddim)")
    if spacing == "trailing":
        if not 0 < num_steps <= num_train:
            raise ValueError(f"{num_steps} trailing timesteps out of {num_train}")
        return [int(t) for t in np.round(np.arange(num_train, 0, -num_train / num_steps)).astype(np.int64) - 1]
    if spacing is not None:
        raise ValueError(f"timestep_spacing {spacing!r}: None (the scheduler's default) or 'trailing'")
    if kind == "dpm++2m":
        return [int(t) for t in np.linspace(0, num_train - 1, num_steps + 1).round()[::-1][:-1].astype(np.int64)]
    ratio = num_train // num_steps
    return [i * ratio + 1 for i in range(num_steps)][::-1]


def coefficient_row(kind: str, ac: torch.Tensor, timesteps: Sequence[int], i: int, eta: float = 0.0):
    """(alpha_t, sigma_t, cx, c0, c1, cn) of step i — one row of the 6-column device table, the eta = 0 table holds its
    first five — all in f64 on the host.  DPM-Solver++ 2M with diffusers' defaults (solver_order 2, midpoint,
    lower_order_final for < 15 steps).  DDIM is DDIMScheduler.step with its `eta`, set_alpha_to_one=False:
        std = eta sqrt((1 - a_prev)/(1 - a_t) (1 - a_t/a_prev))
        x_prev = sqrt(a_prev) x0 + sqrt(1 - a_prev - std^2) eps + std noise,   eps = (x - sqrt(a_t) x0)/sqrt(1 - a_t)
    i.e. x <- cx x + c0 x0 + cn noise with r = sqrt((1 - a_prev - std^2)/(1 - a_t)): cx = r, c0 = sqrt(a_prev) - r sqrt(a_t),
    cn = std (eta = 0: std^2 = 0 leaves every operation of the deterministic step as it is)."""
    ac = ac.double().cpu()
    t = timesteps[i]
    if kind == "ddim":
        tp = t - ac.numel() // len(timesteps)
        a_t = ac[t]
        a_p = ac[tp] if tp >= 0 else ac[0]
        std = float(eta) * ((1 - a_p) / (1 - a_t) * (1 - a_t / a_p)).sqrt()
        r = ((1 - a_p - std ** 2) / (1 - a_t)).sqrt()
        return (float(a_t.sqrt()), float((1 - a_t).sqrt()), float(r), float(a_p.sqrt() - r * a_t.sqrt()), 0.0, float(std))
    al, sg = ac.sqrt(), (1 - ac).sqrt()
    lam = al.log() - sg.log()
    n = len(timesteps)
    tp = 0 if i == n - 1 else timesteps[i + 1]
    h = lam[tp] - lam[t]
    cx = sg[tp] / sg[t]
    base = -al[tp] * (torch.exp(-h) - 1.0)
    if i == 0 or (i == n - 1 and n < 15):
        return float(al[t]), float(sg[t]), float(cx), float(base), 0.0, 0.0
    r0 = (lam[t] - lam[timesteps[i - 1]]) / h
    return float(al[t]), float(sg[t]), float(cx), float(base * (1 + 0.5 / r0)), float(-0.5 * base / r0), 0.0


def step_coefficients(kind: str, ac: torch.Tensor, timesteps: Sequence[int], i: int):
    """(cx, c0, c1, alpha_t, sigma_t) of step i at eta = 0 (coefficient_row in the samplers' own order)"""
    a_t, s_t, cx, c0, c1, _ = coefficient_row(kind, ac, timesteps, i)
    return cx, c0, c1, a_t, s_t


def ddim_eta_coefficients(ac: torch.Tensor, timesteps: Sequence[int], i: int, eta: float):
    """(alpha_t, sigma_t, cx, c0, c1, cn) of DDIM step i with the scheduler's `eta`: coefficient_row("ddim", ...)"""
    if eta < 0:
        raise ValueError(f"eta = {eta}: DDIM's eta lies in [0, 1] (0: deterministic, 1: DDPM-like variance)")
    return coefficient_row("ddim", ac, timesteps, i, eta)


def check_eta(kind: str, eta: float) -> bool:
    """True when the step needs the noise term.  DPMSolverMultistepScheduler.step takes no `eta`: the reference's
    prepare_extra_step_kwargs drops it silently there; here asking for it is an error rather than a deterministic run."""
    if eta == 0.0:
        return False
    if kind != "ddim":
        raise ValueError(f"eta = {eta} with the {kind!r} sampler: only DDIM has an eta (the reference's "
                         "DPMSolverMultistepScheduler ignores the argument); use sampler 'ddim' or eta = 0")
    if eta < 0:
        raise ValueError(f"eta = {eta}: DDIM's eta lies in [0, 1]")
    return True


def check_rescale(guidance_rescale: float) -> bool:
    """True when the step needs the rescale factor (phi > 0); phi outside [0, 1] raises (diffusers takes any float: phi
    weighs the rescaled against the plain guided prediction, and nothing outside [0, 1] is a weight)"""
    phi = float(guidance_rescale)
    if not 0.0 <= phi <= 1.0:  # (NaN fails both comparisons)
        raise ValueError(f"guidance_rescale = {guidance_rescale}: it lies in [0, 1] (0: off, 0.7: the paper's value)")
    return phi > 0.0


_BUFFER_RANGE = 0x7fffffff  # bytes a buffer-resource store can address (csrc/common.h VN_REQUIRE_OUT)


def decoder_sample_bytes(vae: sc.VAEConfig, h: int, w: int) -> int:
    """the largest f16 activation of VAEDecoderEngine for ONE sample of latent size h x w: the resnet / upsample outputs
    at each level (up block i runs at h * 2^i with max(its input, its output) channels) and the mid-block attention
    scores (h w x rup(h w, 64))."""
    boc = list(reversed(vae.block_out_channels))
    peak = h * w * ((h * w + 63) // 64 * 64)
    cin = boc[0]
    for i, cout in enumerate(boc):
        peak = max(peak, (h << i) * (w << i) * max(cin, cout))
        if i < len(boc) - 1:  # the upsample conv writes cout channels at twice the resolution
            peak = max(peak, (h << (i + 1)) * (w << (i + 1)) * cout)
        cin = cout
    return 2 * peak


def decode_sub_batch(vae: sc.VAEConfig, h: int, w: int, batch: int) -> int:
    """the largest divisor of `batch` whose decoder activations stay below the buffer-store range (equal sub-batches:
    one decoder engine, no padded pass)"""
    per = decoder_sample_bytes(vae, h, w)
    for d in range(batch, 0, -1):
        if batch % d == 0 and d * per < _BUFFER_RANGE:
            return d
    raise ValueError(f"one {8 * h}x{8 * w} sample needs {per} bytes in one decoder activation: over 2 GiB")


class InferenceEngine:
    def __init__(self, cfg: sc.SDConfig, unet_w: Dict, vae_dec_w: Dict, clip_w: Dict, batch: int, height: int,
                 width: int, mapper_object: Dict[str, torch.Tensor], w_enc_object: torch.Tensor,
                 norm_scale_object: Optional[float], alpha_object: float = 0.2,
                 mapper_view: Optional[Dict[str, torch.Tensor]] = None, w_enc_view: Optional[torch.Tensor] = None,
                 norm_scale_view: Optional[float] = None, alpha_view: float = 0.2, n_view_params: int = 12,
                 unconstrained_object: bool = False, unconstrained_view: bool = False, hidden_object: int = 64,
                 device: str = "cuda", params_object: Optional[torch.Tensor] = None,
                 params_view: Optional[torch.Tensor] = None, object_slot: Optional[torch.Tensor] = None,
                 object_slot_stride: int = 0, legacy_pe_object: Optional[torch.Tensor] = None,
                 enc_dim_object: int = 64, output_bypass_object: bool = True, output_bypass_view: bool = True,
                 per_sample_slots: bool = False):
        """params_object / params_view: flat device buckets to ALIAS instead of copying the state dicts (validation
        during training reads the live parameters); object_slot (+stride) picks one mapper of a multi-object bucket.
        per_sample_slots: every sample picks its own mapper of the bucket (`slots`, written by set_prompts), so B prompts
        about different objects share one sampler graph; object_slot is then unused."""
        self.cfg = cfg
        self.B = batch
        self.dev = device
        nlev = len(cfg.vae.block_out_channels)
        self.h, self.w = height >> (nlev - 1), width >> (nlev - 1)
        self.Lc = cfg.vae.latent_channels
        B, L, D = batch, cfg.clip.max_positions, cfg.clip.hidden_size
        self.L = L
        self.ac = alphas_cumprod(cfg.ddpm)
        # CFG-batched UNet: samples [0,B) unconditional, [B,2B) conditional
        self.unet = UNetEngine(cfg.unet, unet_w, 2 * batch, self.h, self.w, L, device, need_backward=False)
        nl = cfg.unet.n_cross_layers
        self.t_text = torch.zeros(B, dtype=torch.int64, device=device)
        self.ctx_k = torch.zeros((nl, B * L, D), dtype=lib.act_dtype(), device=device)
        self.ctx_v = torch.zeros_like(self.ctx_k)
        po = params_object if params_object is not None else flatten_mapper_state(mapper_object).to(device)
        # device int32[B] the captured text pass reads (the per-sample form of `object_slot`)
        self.slots = torch.zeros(B, dtype=torch.int32, device=device) if per_sample_slots else None
        self.n_object_slots = po.numel() // object_slot_stride if object_slot_stride else 1
        mo = MapperState(po, w_enc_object.to(device).float().contiguous() if legacy_pe_object is None else None,
                         norm_scale_object, alpha_object, hidden=hidden_object, enc_dim=enc_dim_object,
                         unconstrained=unconstrained_object, slot=object_slot, slot_stride=object_slot_stride,
                         legacy_w_pe=(legacy_pe_object.to(device).float().contiguous()
                                      if legacy_pe_object is not None else None),
                         output_bypass=output_bypass_object, slots=self.slots)
        mv = None
        if mapper_view is not None or params_view is not None:
            pv = params_view if params_view is not None else flatten_mapper_state(mapper_view).to(device)
            mv = MapperState(pv, w_enc_view.to(device).float().contiguous(), norm_scale_view, alpha_view,
                             unconstrained=unconstrained_view, output_bypass=output_bypass_view)
        self.text = TextEngine(cfg.clip, clip_w, nl, batch, self.t_text, self.ctx_k, self.ctx_v, None, None, mo, None,
                               mv, None, n_view_params, False, device, need_backward=False)
        self.text.training = False
        # masks exist from the start: set_truncation() then mutates them in place and a captured sampler graph
        # (whose launches bake the mask pointer in) honours a truncation_idx set after the capture
        self.text.ensure_masks()
        # the decoder runs in sub-batches whose largest activation stays inside the 2 GiB range of the buffer stores
        # (B = 8 at 768 x 768 puts 2.4 GB into the 256-channel full-resolution level); the UNet stays at 2B
        self.decode_batch = decode_sub_batch(cfg.vae, self.h, self.w, batch)
        self.decoder = VAEDecoderEngine(cfg.vae, vae_dec_w, self.decode_batch, self.h, self.w, device)
        shape = (batch, self.Lc, self.h, self.w)
        self.x = torch.zeros(shape, dtype=torch.float32, device=device)
        self.m_prev = torch.zeros_like(self.x)
        if self.decode_batch == batch:
            self.image = self.decoder.image
        else:
            self.image = torch.empty((batch,) + tuple(self.decoder.image.shape[1:]), dtype=torch.float32, device=device)
        self.step_idx = torch.zeros(1, dtype=torch.int32, device=device)
        # device tables a captured sampler step reads (row = step_idx): {alpha_t, sigma_t, cx, c0, c1}, timestep
        self.coef_table = torch.zeros((cfg.ddpm.num_train_timesteps, 5), dtype=torch.float32, device=device)
        self.ts_table = torch.zeros((cfg.ddpm.num_train_timesteps,), dtype=torch.int64, device=device)
        # stochastic DDIM (eta > 0): a 6-column table (+ cn) and the per-step variance noise [T][B][Lc][h][w], allocated
        # at the first such call
        self.coef_table6 = torch.zeros((cfg.ddpm.num_train_timesteps, 6), dtype=torch.float32, device=device)
        self.noise_table = None
        # guidance rescale (phi > 0): f[b] f32 [B] and the f64 partials of its reduction, allocated at the first such call
        # (their size is fixed by the engine's shape: once)
        self.rescale_factor = None
        self.rescale_ws = None
        # captured sampler steps by (guidance_scale, vpred, noisy), plus (phi,) when phi > 0: one per (noisy, rescaled) at a
        # time
        self._graphs = {}

    # ------------------------------------------------------------------ conditioning
    def set_negative_prompt(self, input_ids: torch.Tensor):
        """`negative_prompt_embeds` (sd_pipeline_call.py:35-39): the plain text encoder on the negative prompt;
        used as K and V source of every cross-attention layer of the unconditional half."""
        B, L = self.B, self.L
        ids = input_ids.view(-1, L)
        if ids.shape[0] == 1:
            ids = ids.expand(B, L)
        none = torch.full((B,), -1, dtype=torch.int64)
        self.text.set_batch(ids, none, none if self.text.mv is not None else None, None)
        self.t_text.zero_()
        self.text.forward()
        # without a placeholder the bypass variant equals the plain one, and every layer sees the same embedding
        self.unet.ctx_k[:, : B * L].copy_(self.ctx_k)
        self.unet.ctx_v[:, : B * L].copy_(self.ctx_k)

    def set_prompt(self, input_ids, placeholder_object, placeholder_view=None, view_params=None,
                   truncation_idx: Optional[int] = None):
        self.text.set_batch(input_ids, placeholder_object, placeholder_view, view_params)
        self.text.set_truncation(truncation_idx)

    def set_prompts(self, input_ids: torch.Tensor, placeholder_object: torch.Tensor,
                    placeholder_view: Optional[torch.Tensor] = None, view_params: Optional[torch.Tensor] = None,
                    slots: Optional[Sequence[int]] = None, truncation_idx: Optional[Sequence[Optional[int]]] = None):
        """B different prompts, one per sample: input_ids (B, 77), placeholder ids (B,) (-1 = none), view_params (B, nv)
        for the rows with a view token, slots[b] = which mapper of the object bucket sample b uses (needs
        per_sample_slots).  The negative prompt and the guidance scale stay shared by the whole batch."""
        B = self.B
        ids = input_ids.reshape(B, self.L)
        po = placeholder_object.reshape(B).cpu()
        has_obj = po != -1
        if bool(has_obj.any()) and not bool(has_obj.all()):
            raise ValueError("set_prompts: either every prompt of the batch holds an object placeholder or none does")
        if truncation_idx is not None and not isinstance(truncation_idx, int):
            tr = list(truncation_idx)
            if any(t != tr[0] for t in tr):
                raise ValueError(f"set_prompts: one truncation_idx per batch (got {tr})")
            truncation_idx = tr[0]
        if slots is not None:
            if self.slots is None:
                raise ValueError("set_prompts: per-sample object slots need an engine built with per_sample_slots=True")
            s = torch.as_tensor(list(slots), dtype=torch.int32).reshape(-1)
            if s.numel() != B or bool((s < 0).any()) or bool((s >= self.n_object_slots).any()):
                raise ValueError(f"set_prompts: need {B} slots in [0, {self.n_object_slots}), got {s.tolist()}")
            self.slots.copy_(s)
        elif self.slots is not None:
            self.slots.zero_()
        pv = placeholder_view.reshape(B) if placeholder_view is not None else None
        self.text.set_batch(ids, po, pv, view_params)
        self.text.set_truncation(truncation_idx)

    # ------------------------------------------------------------------ the loop
    @torch.no_grad()
    def generate(self, latents: torch.Tensor, num_inference_steps: int = 50, guidance_scale: float = 7.5,
                 kind: str = "dpm++2m", decode: bool = True, use_graph: bool = True, eta: float = 0.0,
                 step_noise: Optional[torch.Tensor] = None, guidance_rescale: float = 0.0,
                 timestep_spacing: Optional[str] = None):
        """latents: (B, 4, h, w) N(0,1) draw (`prepare_latents`, init_noise_sigma = 1 for both samplers).
        eta > 0 (DDIM only): DDIMScheduler.step's variance term, fed from step_noise, f32 [T][B][4][h][w] N(0,1) (one draw
        per sampler step; None: drawn here from torch's global generator, as the scheduler does without a generator).
        guidance_rescale in [0, 1] (diffusers' argument): the guided prediction of each sample is scaled by
        phi std(cond) / std(guided) + 1 - phi before the step; 0 is off and launches what it always did.
        timestep_spacing: None (the schedulers' lists) or "trailing".
        Returns the images f32 [B, H, W, 3] in [0,1] (the array `numpy_to_pil` receives) or the final latents."""
        ts = self._timesteps(kind, num_inference_steps, guidance_scale, timestep_spacing)
        return self._sample(latents, ts, guidance_scale, kind, decode, eta, step_noise, self._own_conditioning, use_graph,
                            guidance_rescale)

    def _timesteps(self, kind, num_inference_steps, guidance_scale, spacing=None):
        if guidance_scale <= 1.0:
            raise ValueError("sd_pipeline_call only defines the classifier-free-guidance branch (guidance_scale > 1)")
        return inference_timesteps(kind, num_inference_steps, self.cfg.ddpm.num_train_timesteps, spacing)

    def _own_conditioning(self, i, t):
        """eager step i at timestep t: the engine's text pass writes the conditional half of the UNet's contexts"""
        B, L = self.B, self.L
        self.t_text.fill_(t)
        self.unet.timesteps.fill_(t)
        self.text.forward()
        self.unet.ctx_k[:, B * L:].copy_(self.ctx_k)
        self.unet.ctx_v[:, B * L:].copy_(self.ctx_v)

    def _sample(self, latents, ts, guidance_scale, kind, decode, eta, step_noise, conditioning, use_graph,
                guidance_rescale=0.0):
        """the sampler loop behind generate() and generate_from_contexts().  conditioning(i, t) sets the timestep and the
        conditional contexts of eager step i; use_graph replays one captured step instead (which runs the engine's own
        text pass: timesteps and step scalars come from device tables).  eta > 0 (`noisy`) swaps the sampler launch for
        its noise-table sibling and nothing else.  guidance_rescale > 0 (`phi`) swaps it for the factor launches and the
        scaled step, which always reads the 6-column table (cn = 0 rows and no noise pointer at eta = 0)."""
        noisy = check_eta(kind, eta)
        phi = float(guidance_rescale) if check_rescale(guidance_rescale) else 0.0
        vpred = self.cfg.ddpm.prediction_type == "v_prediction"
        self._seed(latents)
        if noisy:
            self._load_step_noise(step_noise, len(ts))
        rows = [coefficient_row(kind, self.ac, ts, i, eta) for i in range(len(ts))]
        if phi:
            self._ensure_rescale()
        if use_graph:
            table = self.coef_table6 if noisy or phi else self.coef_table
            table[: len(ts)].copy_(torch.tensor([r[: table.shape[1]] for r in rows], dtype=torch.float32))
            self.ts_table[: len(ts)].copy_(torch.tensor(ts, dtype=torch.int64))
            self.step_idx.zero_()
            # eta itself lives in the table: one graph serves every eta > 0.  phi is a by-value argument of the factor
            # launch like guidance_scale, so it is part of the key; phi = 0 keeps the key it always had
            key = (guidance_scale, vpred, noisy) + ((phi,) if phi else ())
            if key not in self._graphs:
                self._graphs = {k: g for k, g in self._graphs.items() if (k[2], len(k)) != (noisy, len(key))}
                self._graphs[key] = self._capture(guidance_scale, vpred, noisy, phi)
                self.step_idx.zero_()
                self._seed(latents)
            for _ in ts:
                self._graphs[key].replay()
        else:
            B, n = self.B, self.h * self.w
            for i, t in enumerate(ts):
                conditioning(i, t)
                self.unet.forward()
                if phi:
                    ops.cfg_rescale_factor(self.unet.pred, self.rescale_factor, self.rescale_ws, B, self.Lc, n,
                                           guidance_scale, phi)
                    ops.cfg_sampler_step_scaled(self.unet.pred, self.x, self.m_prev, self.unet.x_in,
                                                self.noise_table[i] if noisy else None, self.rescale_factor, B, self.Lc, n,
                                                guidance_scale, *rows[i], vpred)
                elif noisy:
                    ops.cfg_sampler_step_noise(self.unet.pred, self.x, self.m_prev, self.unet.x_in, self.noise_table[i], B,
                                               self.Lc, n, guidance_scale, *rows[i], vpred)
                else:
                    ops.cfg_sampler_step(self.unet.pred, self.x, self.m_prev, self.unet.x_in, B, self.Lc, n,
                                         guidance_scale, *rows[i][:5], vpred)
        return self.decode() if decode else self.x

    def decode(self) -> torch.Tensor:
        """decode self.x into self.image, `decode_batch` samples per decoder pass"""
        db = self.decode_batch
        if db == self.B:
            self.decoder.z_in.copy_(self.x)
            self.decoder.forward()
            return self.image
        for i in range(0, self.B, db):
            self.decoder.z_in.copy_(self.x[i:i + db])
            self.decoder.forward()
            self.image[i:i + db].copy_(self.decoder.image)
        return self.image

    # ------------------------------------------------------------------ the reference's own prompt_embeds contract
    def load_contexts(self, embed) -> None:
        """Write ONE step's conditional conditioning into the UNet's per-layer K / V sources, as the 16 XTIAttenProc
        instances would read it (models/xti_attention_processor.py:27-41): a dict {CONTEXT_TENSOR_l ->  K source,
        CONTEXT_TENSOR_BYPASS_l -> V source (absent: the former)} or one tensor used by every layer for both."""
        B, L, nl = self.B, self.L, self.cfg.unet.n_cross_layers
        ck, cv = self.unet.ctx_k[:, B * L:], self.unet.ctx_v[:, B * L:]

        def rows(t):
            t = torch.as_tensor(t)
            if t.dim() == 2:
                t = t[None]
            if t.shape[0] == 1 and B > 1:
                t = t.expand(B, *t.shape[1:])
            if tuple(t.shape) != (B, L, ck.shape[-1]):
                raise ValueError(f"context of shape {tuple(t.shape)}: expected ({B}, {L}, {ck.shape[-1]})")
            return t.reshape(B * L, -1)

        if isinstance(embed, dict):
            for l in range(nl):
                k = embed[f"CONTEXT_TENSOR_{l}"]
                v = embed.get(f"CONTEXT_TENSOR_BYPASS_{l}", k)
                ck[l].copy_(rows(k))
                cv[l].copy_(rows(v))
        else:
            r = rows(embed)
            for l in range(nl):
                ck[l].copy_(r)
                cv[l].copy_(r)

    @torch.no_grad()
    def generate_from_contexts(self, latents: torch.Tensor, prompt_embeds, num_inference_steps: int = 50,
                               guidance_scale: float = 7.5, kind: str = "dpm++2m", decode: bool = True,
                               eta: float = 0.0, step_noise: Optional[torch.Tensor] = None,
                               guidance_rescale: float = 0.0, timestep_spacing: Optional[str] = None):
        """`sd_pipeline_call` with the conditioning ALREADY computed, exactly as the reference passes it
        (sd_pipeline_call.py:86: `prompt_embeds[i] if type(prompt_embeds) == list else prompt_embeds`): a list of T
        per-step XTI dicts (PromptManager.embed_prompt's return value, prompt_manager.py:79-99), one dict, or one tensor.
        The engine's own text pass is skipped; the negative prompt must have been set (set_negative_prompt)."""
        ts = self._timesteps(kind, num_inference_steps, guidance_scale, timestep_spacing)
        per_step = type(prompt_embeds) == list
        if per_step and len(prompt_embeds) < len(ts):
            raise ValueError(f"{len(prompt_embeds)} per-step prompt embeddings for {len(ts)} sampler steps")
        if not per_step:
            self.load_contexts(prompt_embeds)

        def conditioning(i, t):
            if per_step:
                self.load_contexts(prompt_embeds[i])
            self.unet.timesteps.fill_(t)

        return self._sample(latents, ts, guidance_scale, kind, decode, eta, step_noise, conditioning, use_graph=False,
                            guidance_rescale=guidance_rescale)

    # ------------------------------------------------------------------ guidance rescale (phi > 0)
    def _ensure_rescale(self) -> None:
        if self.rescale_factor is None:
            self.rescale_factor = torch.ones(self.B, dtype=torch.float32, device=self.dev)
            self.rescale_ws = torch.zeros(ops.cfg_rescale_ws_doubles(self.B, self.h * self.w), dtype=torch.float64,
                                          device=self.dev)

    # ------------------------------------------------------------------ stochastic DDIM (eta > 0)
    def _load_step_noise(self, step_noise: Optional[torch.Tensor], T: int) -> None:
        """upload the variance noise of T steps into the device table (grown, never shrunk: a captured step holds its
        address, so a new allocation drops that graph)"""
        shape = (T, self.B, self.Lc, self.h, self.w)
        if step_noise is None:
            step_noise = torch.randn(shape, dtype=torch.float32)
        if tuple(step_noise.shape) != shape or step_noise.dtype != torch.float32:
            raise ValueError(f"step_noise of shape {tuple(step_noise.shape)} {step_noise.dtype}: expected f32 {shape}")
        if self.noise_table is None or self.noise_table.shape[0] < T:
            self.noise_table = torch.empty(shape, dtype=torch.float32, device=self.dev)
            self._graphs = {k: g for k, g in self._graphs.items() if not k[2]}
        self.noise_table[:T].copy_(step_noise)

    def _seed(self, latents):
        B = self.B
        self.x.copy_(latents)
        self.m_prev.zero_()
        self.unet.x_in[:B].copy_(self.x)
        self.unet.x_in[B:].copy_(self.x)

    def _one_step(self, guidance_scale, vpred, noise=False, phi=0.0):
        B, L = self.B, self.L
        ops.table_fill_i64(self.t_text, self.ts_table, self.step_idx)
        ops.table_fill_i64(self.unet.timesteps, self.ts_table, self.step_idx)
        self.text.forward()
        self.unet.ctx_k[:, B * L:].copy_(self.ctx_k)
        self.unet.ctx_v[:, B * L:].copy_(self.ctx_v)
        self.unet.forward()
        if phi:
            ops.cfg_rescale_factor(self.unet.pred, self.rescale_factor, self.rescale_ws, B, self.Lc, self.h * self.w,
                                   guidance_scale, phi)
            ops.cfg_sampler_step_scaled_table(self.unet.pred, self.x, self.m_prev, self.unet.x_in, B, self.Lc,
                                              self.h * self.w, guidance_scale, self.coef_table6,
                                              self.noise_table if noise else None, self.rescale_factor, self.step_idx,
                                              vpred)
        elif noise:
            ops.cfg_sampler_step_noise_table(self.unet.pred, self.x, self.m_prev, self.unet.x_in, B, self.Lc,
                                             self.h * self.w, guidance_scale, self.coef_table6, self.noise_table,
                                             self.step_idx, vpred)
        else:
            ops.cfg_sampler_step_table(self.unet.pred, self.x, self.m_prev, self.unet.x_in, B, self.Lc, self.h * self.w,
                                       guidance_scale, self.coef_table, self.step_idx, vpred)
        ops.counter_advance(self.step_idx)

    def _capture(self, guidance_scale, vpred, noise=False, phi=0.0):
        """one sampler step as a graph (its warm-up run is a real step: the caller re-seeds x afterwards)"""
        step = partial(self._one_step, guidance_scale, vpred, noise, phi)
        return capture_graphs([step], warmup=step)[0]

    def memory_bytes(self) -> int:
        noise = 0 if self.noise_table is None else self.noise_table.numel() * 4
        rescale = 0 if self.rescale_factor is None else self.rescale_factor.numel() * 4 + self.rescale_ws.numel() * 8
        return self.unet.bytes + self.text.bytes + self.decoder.bytes + noise + rescale
