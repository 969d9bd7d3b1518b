"""One textual-inversion optimisation step on one GPU as a single replayable launch schedule.

Mirrors the loop body of `Coach.train` (training/coach.py:154-231):

    latents = vae.encode(px).latent_dist.sample() * scaling_factor        -> VAEEncoderEngine + sample_add_noise
    noise, timesteps, noisy = randn_like, randint, scheduler.add_noise    -> device RNG + sample_add_noise
    _hs = get_text_conditioning(...)                                      -> TextEngine.forward
    model_pred = unet(noisy, timesteps, _hs).sample                       -> UNetEngine.forward
    loss = mse_loss(model_pred.float(), target.float())                   -> mse_loss_grad
    accelerator.backward(loss)  (GradScaler-scaled under fp16)            -> UNetEngine.backward + TextEngine.backward
    optimizer.step(); zero_grad()                                         -> adamw_flat (flat bucket)

Everything that varies per step lives in device memory (RNG counter, optimizer step, loss scale,
learning rate), so the step is captured once into a hipGraph and replayed.  Deliberate
deviations from the reference, all documented in DESIGN.md: the placeholder-embedding "restore"
(coach.py:222-229) is dropped (the table is never in the optimizer); noise/timesteps come from a
counter-hash device RNG instead of torch's Philox stream; data-parallel training all-reduces one
flat mapper-gradient bucket instead of wrapping the text encoder in DDP.
"""
from __future__ import annotations

from functools import partial
from typing import Dict, List, Optional

import torch

from .. import ops
from .. import sd_config as sc
from .graphs import capture_graphs
from .text import MapperState, TextEngine
from .unet import UNetEngine
from .vae import VAEEncoderEngine


def alphas_cumprod(cfg: sc.DDPMConfig) -> torch.Tensor:
    """DDPMScheduler(beta_schedule='scaled_linear'): betas = linspace(sqrt(b0), sqrt(b1), T)^2."""
    betas = torch.linspace(cfg.beta_start ** 0.5, cfg.beta_end ** 0.5, cfg.num_train_timesteps,
                           dtype=torch.float32) ** 2
    return torch.cumprod(1.0 - betas, dim=0)


class TrainStepEngine:
    def __init__(self, cfg: sc.SDConfig, unet_w: Dict, vae_w: Dict, clip_w: Dict, batch: int, height: int,
                 width: int, mapper_object: Dict[str, torch.Tensor], w_enc_object: torch.Tensor,
                 norm_scale_object: Optional[float], alpha_object: float = 0.2,
                 mapper_view: Optional[Dict[str, torch.Tensor]] = None, w_enc_view: Optional[torch.Tensor] = None,
                 norm_scale_view: Optional[float] = None, alpha_view: float = 0.2, train_view: bool = True,
                 n_view_params: int = 12, lr: float = 1e-3, betas=(0.9, 0.999), adam_eps: float = 1e-8,
                 weight_decay: float = 1e-2, loss_scale: Optional[float] = None, growth_interval: int = 2000,
                 seed: int = 0, world_size: int = 1, device_rng: bool = True, device: str = "cuda",
                 need_backward: bool = True, grad_accum: int = 1, overlap: bool = False,
                 unconstrained_object: bool = False, unconstrained_view: bool = False,
                 nested_dropout_prob: float = 0.0, hidden_object: int = 64,
                 legacy_pe_object: Optional[torch.Tensor] = None, enc_dim_object: int = 64,
                 output_bypass_object: bool = True, output_bypass_view: bool = True, exchange=None,
                 moment_cache_images: int = 0, max_grad_norm: Optional[float] = None, telemetry_rows: int = 0,
                 snr_gamma: Optional[float] = None, noise_offset: Optional[float] = None,
                 ema_decay: Optional[float] = None, ema_update_after_step: int = 0,
                 ema_warmup_power: Optional[float] = None, loss_mask: bool = False, loss_mask_background: float = 0.0):
        """mapper_object: one mapper state_dict, or a list of them (learnable_mode 3: one object mapper per
        scene, `mapper_object_lookup`, training/coach.py:505-552) — `set_batch(object_index=k)` picks the one
        the batch trains.
        max_grad_norm: clip the (unscaled, mean) mapper gradient to this global L2 norm before AdamW, as
        torch.nn.utils.clip_grad_norm_ after GradScaler.unscale_ would.  telemetry_rows: > 0 keeps a device ring of that
        many micro-steps (timesteps, per-sample losses, gradient norms, loss scale, lr, skipped steps) for
        read_telemetry().  Both off: the step enqueues the launches it always did.
        snr_gamma: Min-SNR-gamma weighting of the training loss (diffusers' --snr_gamma; inf is legal: every weight 1).
        noise_offset: offset noise, noise += noise_offset * randn(B, C, 1, 1) (diffusers' --noise_offset).  Both are None
        or > 0 and touch the TRAINING objective only: eval_losses() stays the plain MSE on plain noise, and the ring's
        per-sample losses stay unweighted.  Both off: the step enqueues the launches it always did.
        ema_decay: keep an exponential moving average of the bucket on the device, updated at the end of every applied
        optimizer step (diffusers' EMAModel; None or the cap of the decay, in (0, 1)).  ema_update_after_step delays it,
        ema_warmup_power (None or > 0) picks the 1 - (1 + s)^(-power) ramp over (1 + s) / (10 + s).  The average only reads
        `params`; ema_weights() swaps it in for evaluation.  Off: no buffer, no launch.
        loss_mask: weight every latent pixel of the training loss by the sample's object mask (`loss_weights`, f32
        [B][h*w], one row per sample written by set_loss_mask() outside the captured step; ones until then), each sample
        normalised by its own mask mass.  loss_mask_background in [0, 1]: the weight of a background pixel before the
        normalisation.  One loss launch swapped for its weighted sibling, none added; eval_losses() stays unmasked.  Off:
        no buffer, and the step enqueues the launches it always did."""
        from .text import flatten_mapper_state
        # the average's settings, refused before anything is built.  (`not a < x < b` also refuses nan)
        if ema_decay is not None and not 0.0 < float(ema_decay) < 1.0:
            raise ValueError(f"ema_decay must be in (0, 1) (is {ema_decay!r}); None turns the average off")
        if ema_warmup_power is not None and not 0.0 < float(ema_warmup_power) < float("inf"):
            raise ValueError(f"ema_warmup_power must be > 0 and finite (is {ema_warmup_power!r}); None is the (1+s)/(10+s) ramp")
        if int(ema_update_after_step) != ema_update_after_step or not 0 <= ema_update_after_step < 2 ** 24:
            raise ValueError(f"ema_update_after_step must be an integer in [0, 2^24) (is {ema_update_after_step!r})")
        if ema_decay is None and (ema_update_after_step or ema_warmup_power is not None):
            raise ValueError("ema_update_after_step / ema_warmup_power need ema_decay")
        if ema_decay is not None and not need_backward:
            raise ValueError("ema_decay needs an engine that trains")
        # the object mask's settings
        if not 0.0 <= float(loss_mask_background) <= 1.0:
            raise ValueError(f"loss_mask_background must be in [0, 1] (is {loss_mask_background!r})")
        if not loss_mask and float(loss_mask_background) != 0.0:
            raise ValueError("loss_mask_background needs loss_mask")
        if loss_mask and not need_backward:
            raise ValueError("loss_mask needs an engine that trains")
        self.cfg = cfg
        self.B, self.H, self.W = batch, height, width
        self.dev = device
        self.world_size = world_size
        # the exchange step.  On the nccl (= RCCL) backend it is a call into the library's own communicator
        # (vneti_allreduce_flat, csrc/comm.hip): stream-ordered and capturable, so the data-parallel step is the SAME single
        # hipGraph as the one-GPU step plus one collective node (capture()).  VNETI_RCCL_DIRECT=0, the gloo backend (CPU
        # tests, two ranks on one GPU) and any failure to build the communicator fall back to torch.distributed.all_reduce
        # issued from the host between two graphs.  `exchange` may also be handed in (tests: a world-size-1 communicator).
        self.exchange = exchange
        if world_size > 1 and exchange is None:
            import os
            import torch.distributed as dist
            if os.environ.get("VNETI_RCCL_DIRECT", "1") != "0" and dist.is_initialized() and dist.get_backend() == "nccl":
                from ..parallel import enable_direct_rccl
                try:  # the outcome is agreed over the process group (RcclComm): every rank raises, or none does
                    self.exchange = enable_direct_rccl()
                except RuntimeError as err:  # loud, not fatal: torch's communicator does the same collective
                    if os.environ.get("VNETI_REQUIRE_ONE_GRAPH", "0") == "1":
                        raise
                    import warnings
                    warnings.warn(f"library RCCL communicator unavailable ({err}); using torch.distributed.all_reduce")
        self.device_rng = device_rng
        if loss_scale is None:
            # accelerate creates a GradScaler for mixed_precision fp16 only; bf16 has f32's exponent range: a STATIC scale of 1
            # (growth_interval 0: never halved, never grown — the non-finite check and the skip-step logic stay, they
            # cost one tiny kernel)
            from .. import lib
            loss_scale = 1.0 if lib.precision() == "bf16" else 65536.0
            if lib.precision() == "bf16":
                growth_interval = 0
        self.growth_interval = growth_interval
        nlev = len(cfg.vae.block_out_channels)
        self.h, self.w = height >> (nlev - 1), width >> (nlev - 1)
        Lc = cfg.vae.latent_channels
        D = cfg.clip.hidden_size
        # ---- trainable state: one flat f32 bucket [object mapper 0 .. K-1 | view mapper] ----
        objs = list(mapper_object) if isinstance(mapper_object, (list, tuple)) else [mapper_object]
        flats = [flatten_mapper_state(sd) for sd in objs]
        self.n_objects = len(flats)
        self.n_obj = flats[0].numel()  # floats per object mapper
        assert all(f.numel() == self.n_obj for f in flats), "object mappers must share one architecture"
        flat_v = flatten_mapper_state(mapper_view) if (mapper_view is not None and train_view) else None
        n_all_obj = self.n_obj * self.n_objects
        n = n_all_obj + (flat_v.numel() if flat_v is not None else 0)
        self.params = torch.zeros(n, dtype=torch.float32, device=device)
        self.params[:n_all_obj].copy_(torch.cat(flats))
        if flat_v is not None:
            self.params[n_all_obj:].copy_(flat_v)
        self.grads = torch.zeros_like(self.params)
        self.exp_avg = torch.zeros_like(self.params)
        self.exp_avg_sq = torch.zeros_like(self.params)
        self.n_all_obj = n_all_obj
        # device-side choice of the object mapper (graph-replay safe) + torch's per-parameter Adam step counts
        self.obj_slot = torch.zeros(1, dtype=torch.int32, device=device)
        self.seg_step = torch.zeros(self.n_objects, dtype=torch.int32, device=device)
        self.active_object = 0
        multi = self.n_objects > 1
        # RNG state first: nested dropout draws from it
        self.rng_state = torch.tensor([seed & 0x7FFFFFFF, 0], dtype=torch.int32, device=device)
        # legacy_pe_object: the [1024][2] frequencies of a legacy (arch_view_net <= 14) object mapper; its state dict then
        # carries input_layer.* and enc_dim_object = anchors * layers = 160 (models/neti_mapper.py:90-163)
        mo = MapperState(self.params[:n_all_obj],
                         w_enc_object.to(device).float().contiguous() if legacy_pe_object is None else None,
                         norm_scale_object, alpha_object, hidden=hidden_object, enc_dim=enc_dim_object,
                         unconstrained=unconstrained_object,
                         nested_dropout_prob=nested_dropout_prob, slot=self.obj_slot if multi else None,
                         slot_stride=self.n_obj if multi else 0,
                         legacy_w_pe=(legacy_pe_object.to(device).float().contiguous()
                                      if legacy_pe_object is not None else None),
                         output_bypass=output_bypass_object)
        mv, gv = None, None
        if mapper_view is not None:
            if flat_v is not None:
                pv, gv = self.params[n_all_obj:], self.grads[n_all_obj:]
            else:  # frozen pretrained view mapper (learnable_mode 4/5)
                pv = flatten_mapper_state(mapper_view).to(device)
            mv = MapperState(pv, w_enc_view.to(device).float().contiguous(), norm_scale_view, alpha_view,
                             unconstrained=unconstrained_view,
                             nested_dropout_prob=nested_dropout_prob if flat_v is not None else 0.0,
                             output_bypass=output_bypass_view)
        # ---- device-resident scalars ----
        self.grad_accum = grad_accum
        # accelerate scales each micro-loss by 1/accum and DDP averages over ranks: fold both into AdamW
        self.hyper = torch.tensor([lr, betas[0], betas[1], adam_eps, weight_decay, float(world_size * grad_accum)],
                                  dtype=torch.float32, device=device)
        self.scaler = torch.tensor([loss_scale, 0.0, 0.0], dtype=torch.float32, device=device)
        self.opt_step = torch.zeros(1, dtype=torch.int32, device=device)
        self.loss_sum = torch.zeros(1, dtype=torch.float32, device=device)
        self.ac = alphas_cumprod(cfg.ddpm).to(device)
        # ---- engines ----  (every rank builds these three in this order: the one place where the autotuner's picks are
        # shared by a broadcast — rank-0-only engines such as the validator's stay outside, parallel.shared_picks)
        from ..parallel import shared_picks
        with shared_picks():
            self.unet = UNetEngine(cfg.unet, unet_w, batch, self.h, self.w, cfg.clip.max_positions, device, need_backward)
            self.vae = VAEEncoderEngine(cfg.vae, vae_w, batch, height, width, device)
            self.text = TextEngine(cfg.clip, clip_w, cfg.unet.n_cross_layers, batch, self.unet.timesteps, self.unet.ctx_k,
                                   self.unet.ctx_v, self.unet.dctx_k, self.unet.dctx_v, mo, self.grads[:n_all_obj], mv,
                                   gv, n_view_params, train_view, device, need_backward, rng_state=self.rng_state)
        self.timesteps = self.unet.timesteps
        self.pixel_values = self.vae.x_in
        shape = (batch, Lc, self.h, self.w)
        self.eps = torch.zeros(shape, dtype=torch.float32, device=device)
        self.noise = torch.zeros(shape, dtype=torch.float32, device=device)
        self.latents = torch.zeros(shape, dtype=torch.float32, device=device)
        self.target = torch.zeros(shape, dtype=torch.float32, device=device)
        # ---- optional cache of the VAE posterior moments per dataset image (deterministic datasets only: the CALLER vouches
        # for that — compat/coach.py enables it for augmentation_key 0).  `latent_dist.sample()` is still drawn every step.
        self.n_cache = int(moment_cache_images)
        if self.n_cache:
            hw2 = self.h * self.w
            self.mcache = torch.zeros(self.n_cache, hw2, 2 * Lc, dtype=self.vae.moments.dtype, device=device)
            self.img_idx = torch.zeros(batch, dtype=torch.int64, device=device)
            self._cached_images = set()   # host mirror: which slots hold moments
            self._batch_cached = False    # does the batch set by set_batch() consist of cached images only
            self._batch_images = ()
        self.graph_a_c = self.graph_acc_c = None  # the captured step without the VAE encoder (moments from the cache)
        # held-out evaluation (eval_losses): per-sample losses and the scratch of their two-stage reduction
        self.eval_out = torch.zeros(batch, dtype=torch.float32, device=device)
        self.eval_ws = torch.zeros(ops.mse_loss_per_sample_ws_floats(batch, self.h * self.w), dtype=torch.float32,
                                   device=device)
        self.eval_out_masked = None  # eval_losses(weights=): allocated on first use
        self.graph_eval = None
        from .staging import HostStager
        self.stager = HostStager()
        self.need_backward = need_backward
        self.overlap = overlap
        self.side = torch.cuda.Stream() if overlap else None
        self.graph_a = self.graph_b = self.graph_acc = None
        self.exchange_in_graph = False
        self._reduce_stage = None  # packed [scene segment | view mapper] gradients of a several-object exchange
        self.last_reduce_bytes = 0
        self.micro = 0
        self._eval_batch = False  # the current batch was set for eval_losses(): not to be trained on
        self.n_loss = batch * Lc * self.h * self.w
        # ---- gradient norm / clipping / per-step record.  None of it is trainer state
        if max_grad_norm is not None and not float(max_grad_norm) > 0.0:
            raise ValueError(f"max_grad_norm must be > 0 (is {max_grad_norm!r}); None turns clipping off")
        if telemetry_rows < 0 or (telemetry_rows and not need_backward):
            raise ValueError("telemetry_rows must be >= 0, and the record needs an engine that trains")
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.telemetry_rows = int(telemetry_rows)
        self._norm_path = self.max_grad_norm is not None or self.telemetry_rows > 0
        self._ephemeral = ()  # what _capture() snapshots and restores besides the trainer state
        if self._norm_path:
            multi_obj = self.n_objects > 1
            n_view = self.params.numel() - n_all_obj
            self.max_norm_dev = torch.tensor([self.max_grad_norm or 0.0], dtype=torch.float32, device=device)
            self.norm_out = torch.zeros(ops.NORM_OUT_FLOATS, dtype=torch.float32, device=device)
            self._n_ws_obj = ops.grad_sumsq_ws_doubles(self.n_obj, 1) if multi_obj else ops.grad_sumsq_ws_doubles(n_all_obj)
            self._n_ws_view = ops.grad_sumsq_ws_doubles(n_view) if n_view else 0
            self.norm_ws_obj = torch.zeros(self._n_ws_obj, dtype=torch.float64, device=device)
            self.norm_ws_view = torch.zeros(self._n_ws_view, dtype=torch.float64, device=device) if n_view else None
            self._ephemeral = (self.norm_out,)
        self.tele_ring = self.tele_count = None
        if self.telemetry_rows:
            # ONE buffer [counter, 3 x pad | ring]: read_telemetry() is one device -> host copy
            W = ops.telemetry_row_floats(batch)
            self.tele_buf = torch.zeros(4 + self.telemetry_rows * W, dtype=torch.int32, device=device)
            self.tele_count = self.tele_buf[0:1]
            self.tele_ring = self.tele_buf[4:].view(torch.float32)
            self.rec_loss = torch.zeros(batch, dtype=torch.float32, device=device)
            self.rec_ws = torch.zeros_like(self.eval_ws)
            self._tele_read = 0       # the counter at the last read_telemetry()
            self.telemetry_lost = 0   # micro-steps overwritten before they were read, over the engine's life
            self._ephemeral += (self.tele_buf,)
        # ---- the training objective's options.  Neither is trainer state: the offset draw is stream 5 of
        # rng_state.  (`not x > 0` also refuses nan)
        if snr_gamma is not None and not float(snr_gamma) > 0.0:
            raise ValueError(f"snr_gamma must be > 0, inf allowed (is {snr_gamma!r}); None turns the weighting off")
        if noise_offset is not None and not 0.0 < float(noise_offset) < float("inf"):
            raise ValueError(f"noise_offset must be > 0 and finite (is {noise_offset!r}); None turns offset noise off")
        self.snr_gamma = None if snr_gamma is None else float(snr_gamma)
        self.noise_offset = None if noise_offset is None else float(noise_offset)
        self.offset_noise = None  # f32 [B][Lc]: one draw per (sample, channel), allocated before any capture
        if self.noise_offset is not None:
            self.offset_noise = torch.zeros(batch, Lc, dtype=torch.float32, device=device)
            self._offset_noise_set = False  # host-supplied randomness: has set_noise() delivered the draw
        # ---- the average of the bucket (settings checked above).  `ema` and `ema_count` ARE trainer state;
        # ema_coef is scratch
        self.ema_decay = None if ema_decay is None else float(ema_decay)
        self.ema_update_after_step = int(ema_update_after_step) or None  # (None where unset: the _WHEN_SET rule)
        self.ema_warmup_power = None if ema_warmup_power is None else float(ema_warmup_power)
        self.ema = self.ema_count = None
        self._ema_swapped = False  # inside ema_weights(): `params` holds the average
        if self.ema_decay is not None:
            self.ema = self.params.clone()
            self.ema_count = torch.zeros(2, dtype=torch.int32, device=device)  # {n_updates, last_opt_step}
            self.ema_hyper = torch.tensor([self.ema_decay, float(int(ema_update_after_step)), self.ema_warmup_power or 0.0,
                                           0.0], dtype=torch.float32, device=device)
            self.ema_coef = torch.zeros(ops.EMA_COEF_FLOATS, dtype=torch.float32, device=device)
            self._STATE = type(self)._STATE + ("ema", "ema_count")  # (this instance's: a state without EMA has neither)
        # ---- the object-masked objective (settings checked above).  The table is NOT trainer state: it is
        # rewritten for every batch, like the pixels.  (None where unset: the _WHEN_SET rule)
        self.loss_mask = True if loss_mask else None
        self.loss_mask_background = float(loss_mask_background) or None
        self.loss_weights = self._mask_ws = None
        self._mask_in = None  # uint8 [B][H][W]: where set_loss_masks() uploads a host batch (allocated on first use)
        self.vae_factor = 1 << (nlev - 1)
        if loss_mask:
            self.loss_weights = torch.ones(batch, self.h * self.w, dtype=torch.float32, device=device)
            self._mask_ws = torch.zeros(ops.loss_weights_from_mask_ws_ints(height, width, self.vae_factor), dtype=torch.int32,
                                        device=device)

    # ------------------------------------------------------------------ inputs
    def set_batch(self, pixel_values, input_ids, placeholder_object, placeholder_view=None, view_params=None,
                  object_index: int = 0, image_idx=None, for_eval: bool = False):
        """object_index: which object mapper this batch trains (a batch is single-scene:
        models/net_clip_text_embedding.py:67-76 asserts one placeholder id and looks its mapper up).
        for_eval: a batch for eval_losses(): its images are no dataset items, so the moment cache is neither consulted nor
        told about them (image_idx is ignored).  Such a batch is not trained on: step() refuses until the next set_batch()
        (with a cache, the encoder's moments would otherwise land in the slots of the previous training batch)."""
        if not 0 <= object_index < self.n_objects:
            raise ValueError(f"object_index {object_index} out of range (have {self.n_objects} object mappers)")
        if self.micro != 0 and object_index != self.active_object:
            raise ValueError("the object mapper may not change inside a gradient-accumulation group")
        self.active_object = object_index
        self.obj_slot.fill_(object_index)
        self._eval_batch = bool(for_eval)
        # every host -> device upload of the batch goes through a pinned staging slot (engine/staging.py): the host does not
        # wait for the previous step's graph, it enqueues the copies behind it and moves on
        st = self.stager
        st.begin()
        try:
            if self.n_cache and for_eval:
                self._batch_images, self._batch_cached = (), False  # no slot of the cache belongs to this batch
            elif self.n_cache:
                if image_idx is None:
                    raise ValueError("the moment cache needs the dataset index of every image of the batch (image_idx)")
                ids = tuple(int(i) for i in image_idx)
                if min(ids) < 0 or max(ids) >= self.n_cache:
                    raise ValueError(f"image_idx {ids} outside the moment cache (0..{self.n_cache - 1})")
                st.upload("img_idx", self.img_idx, torch.as_tensor(ids, dtype=torch.int64))
                self._batch_images = ids
                self._batch_cached = all(i in self._cached_images for i in ids)
            self.text.set_batch(input_ids, placeholder_object, placeholder_view, view_params, upload=st.upload)
            if pixel_values is not None:  # None: the device input pipeline already wrote self.pixel_values
                st.upload("pixels", self.pixel_values, pixel_values)  # (large: a blocking copy, issued LAST)
        finally:
            st.end()

    MASK_THRESHOLD = 3  # process_imgs' binarisation `mask / 255 > 0.01` on uint8: value >= 3

    def set_loss_mask(self, b: int, mask_u8: torch.Tensor, H: int, W: int, pixel_stride: int = 1):
        """row b of `loss_weights` from sample b's object mask: a uint8 device image [H][W][pixel_stride] (channel 0 is
        read; stride 3 is what DeviceImagePipeline.run leaves behind) at the engine's training resolution.  Two small
        launches on the current stream, OUTSIDE the captured step (which only reads the table), like the pixel upload."""
        if self.loss_weights is None:
            raise RuntimeError("set_loss_mask(): this engine was built without loss_mask")
        if not 0 <= b < self.B:
            raise ValueError(f"set_loss_mask(): sample {b} outside the batch of {self.B}")
        if (H, W) != (self.H, self.W):
            raise ValueError(f"set_loss_mask(): a {H}x{W} mask gives a {H // self.vae_factor}x{W // self.vae_factor} latent, "
                             f"this engine's is {self.h}x{self.w} ({self.H}x{self.W} pixels)")
        if mask_u8.dtype != torch.uint8 or not mask_u8.is_cuda or mask_u8.numel() < H * W * pixel_stride:
            raise ValueError("set_loss_mask(): the mask is a uint8 device tensor of H * W * pixel_stride bytes")
        ops.loss_weights_from_mask(mask_u8, H, W, pixel_stride, self.vae_factor, self.MASK_THRESHOLD,
                                   self.loss_mask_background or 0.0, self.loss_weights, b, self._mask_ws)

    def set_loss_masks(self, masks_u8: torch.Tensor):
        """the batch's masks from the host: uint8 [B][H][W], uploaded through the pinned stager, then one set_loss_mask()
        per sample"""
        if self.loss_weights is None:
            raise RuntimeError("set_loss_masks(): this engine was built without loss_mask")
        if tuple(masks_u8.shape) != (self.B, self.H, self.W) or masks_u8.dtype != torch.uint8:
            raise ValueError(f"set_loss_masks(): expected uint8 {(self.B, self.H, self.W)}, got {masks_u8.dtype} "
                             f"{tuple(masks_u8.shape)}")
        if self._mask_in is None:
            self._mask_in = torch.zeros(self.B, self.H, self.W, dtype=torch.uint8, device=self.dev)
        st = self.stager
        st.begin()
        try:
            st.upload("loss_masks", self._mask_in, masks_u8)
        finally:
            st.end()
        for b in range(self.B):
            self.set_loss_mask(b, self._mask_in[b], self.H, self.W, 1)

    def train(self, mode: bool = True):
        """nested dropout is a training-time feature (neti_mapper.py:403); eval() turns the draws off.
        (a captured graph keeps the mode it was captured in)"""
        self.text.training = mode
        return self

    def object_params(self, k: int = 0) -> torch.Tensor:
        return self.params[k * self.n_obj:(k + 1) * self.n_obj]

    def view_params_flat(self) -> torch.Tensor:
        return self.params[self.n_all_obj:]

    def set_noise(self, eps, noise, timesteps, offset_noise=None):
        """host-supplied randomness (parity tests: identical values for the oracle and the GPU).  offset_noise: the (B, Lc)
        draw of offset noise: required by an engine built with noise_offset and without the device RNG (with it, stream 5
        draws it in the step, and the held-out evaluation, which calls this, never reads it); refused by an engine without
        noise_offset."""
        if offset_noise is None and self.noise_offset is not None and not self.device_rng:
            raise ValueError("set_noise(): an engine with noise_offset and device_rng=False needs the (B, Lc) offset_noise draw")
        if offset_noise is not None and self.noise_offset is None:
            raise ValueError("set_noise(): offset_noise given, but this engine has no noise_offset")
        if offset_noise is not None:
            if tuple(offset_noise.shape) != tuple(self.offset_noise.shape):
                raise ValueError(f"set_noise(): offset_noise has shape {tuple(offset_noise.shape)}, expected "
                                 f"{tuple(self.offset_noise.shape)}")
            self.offset_noise.copy_(offset_noise)
            self._offset_noise_set = True
        self.eps.copy_(eps)
        self.noise.copy_(noise)
        self.timesteps.copy_(timesteps)

    def set_lr(self, lr: float):
        st = self.stager  # (a scalar write `hyper[0] = lr` is a blocking upload too)
        st.begin()
        st.upload("lr", self.hyper[0:1], torch.tensor([lr], dtype=torch.float32))
        st.end()

    # ------------------------------------------------------------------ trainer state (resumable training)
    _STATE = ("params", "exp_avg", "exp_avg_sq", "opt_step", "seg_step", "scaler", "rng_state", "hyper")

    # described only where set: older states read as "unset"
    _WHEN_SET = ("max_grad_norm", "snr_gamma", "noise_offset", "ema_decay", "ema_update_after_step", "ema_warmup_power",
                 "loss_mask", "loss_mask_background")

    def _describe(self) -> Dict:
        from .. import lib
        return {"n_params": self.params.numel(), "n_objects": self.n_objects, "n_obj": self.n_obj,
                "view_in_bucket": self.params.numel() > self.n_all_obj, "grad_accum": self.grad_accum,
                "world_size": self.world_size, "precision": lib.precision(),
                **{k: getattr(self, k) for k in self._WHEN_SET if getattr(self, k) is not None}}

    def state_dict(self) -> Dict:
        """CPU copies of everything the captured step reads and writes in place — the set `_capture` snapshots around its
        warm-up, plus the hyper-parameters — and a description `load_state_dict` validates.  Gradients are not state: the
        first micro-step of a group overwrites them.  The VAE moment cache is not state either (D14: a hit and a miss are
        bit-identical)."""
        self._refuse_ema_weights("state_dict()")
        if self.micro != 0:
            raise RuntimeError(f"state_dict() inside a gradient-accumulation group (micro-step {self.micro} of "
                               f"{self.grad_accum}): the accumulated gradients are not part of the state")
        sd = {name: getattr(self, name).detach().cpu().clone() for name in self._STATE}
        sd["meta"] = self._describe()
        return sd

    def load_state_dict(self, sd: Dict):
        """copies IN PLACE (the captured graphs hold these buffers' addresses): valid before capture() — whose warm-up
        snapshot then carries the loaded values — and after it, without re-capture.  `hyper` comes back as saved, lr
        included; a caller with a schedule rewrites the lr through set_lr()."""
        self._refuse_ema_weights("load_state_dict()")
        if self.micro != 0:
            raise RuntimeError("load_state_dict() inside a gradient-accumulation group")
        want, have = self._describe(), sd.get("meta", {})
        bad = [f"{k}: saved {have.get(k)!r}, this engine {v!r}" for k, v in want.items() if have.get(k) != v]
        # (a state from before f7 / f8 / f9 / f11 has no such keys: unclipped, unweighted, no offset noise, no average, no mask)
        bad += [f"{k}: saved {have[k]!r}, this engine None" for k in self._WHEN_SET if k in have and k not in want]
        bad += [f"{name}: saved shape {tuple(sd[name].shape) if name in sd else None}, this engine "
                f"{tuple(getattr(self, name).shape)}" for name in self._STATE
                if name not in sd or sd[name].shape != getattr(self, name).shape or sd[name].dtype != getattr(self, name).dtype]
        if bad:
            raise ValueError("trainer state does not fit this engine: " + "; ".join(bad))
        for name in self._STATE:
            getattr(self, name).copy_(sd[name])
        torch.cuda.current_stream().synchronize()

    # ------------------------------------------------------------------ the step
    def forward_backward(self, accumulate: bool = False, cached: bool = False):
        """cached: the batch's VAE moments come out of the moment cache (no encoder launches); otherwise the encoder runs
        and, with a cache, its moments are stored at the batch's image slots."""
        self._refuse_ema_weights("forward_backward()")
        B, Lc, hw = self.B, self.cfg.vae.latent_channels, self.h * self.w
        self.text.accumulate_grads = accumulate
        if self.device_rng:
            ops.rng_advance(self.rng_state)
            ops.rng_fill_randint(self.timesteps, self.cfg.ddpm.num_train_timesteps, self.rng_state, 0)
            ops.rng_fill_normal(self.eps, self.rng_state, 1)
            ops.rng_fill_normal(self.noise, self.rng_state, 2)
            if self.noise_offset is not None:  # (streams 3 and 4 are the nested-dropout masks of the two mappers)
                ops.rng_fill_normal(self.offset_noise, self.rng_state, 5)
        elif self.noise_offset is not None and not self._offset_noise_set:
            raise RuntimeError("noise_offset without the device RNG: set_noise(..., offset_noise=) has to deliver the draw")
        self._forward_half(cached, bool(self.n_cache), fork=self.overlap, noise_offset=self.noise_offset)
        self.loss_sum.zero_()
        vpred = self.cfg.ddpm.prediction_type == "v_prediction"
        if self.loss_weights is not None:  # (the same single launch, with the mask's weights and the null-able SNR pair)
            snr = {} if self.snr_gamma is None else dict(t=self.timesteps, ac=self.ac, gamma=self.snr_gamma, vpred=vpred)
            ops.mse_loss_grad_weighted(self.unet.pred, self.target, self.unet.dpred, self.loss_sum, self.scaler,
                                       self.loss_weights, B, Lc, hw, **snr)
        elif self.snr_gamma is None:
            ops.mse_loss_grad(self.unet.pred, self.target, self.unet.dpred, self.loss_sum, self.scaler, B, Lc, hw)
        else:
            ops.mse_loss_grad_snr(self.unet.pred, self.target, self.unet.dpred, self.loss_sum, self.scaler, B, Lc, hw,
                                  self.timesteps, self.ac, self.snr_gamma, vpred)
        if self.telemetry_rows:  # the micro-step's row: timesteps + the deterministic per-sample losses, then count += 1
            if self.loss_weights is not None:  # (the masked ones: what the step minimises, before the Min-SNR weight)
                ops.mse_loss_per_sample_weighted(self.unet.pred, self.target, self.loss_weights, self.rec_loss, self.rec_ws,
                                                 B, Lc, hw)
            else:
                ops.mse_loss_per_sample(self.unet.pred, self.target, self.rec_loss, self.rec_ws, B, Lc, hw)
            ops.train_record(self.tele_ring, self.tele_count, self.telemetry_rows, not accumulate, self.timesteps,
                             self.rec_loss, B)
        if self.need_backward:
            self.unet.backward()
            self.text.backward()

    def _forward_half(self, cached: bool, write_cache: bool, fork: bool = False, noise_offset: Optional[float] = None):
        """VAE moments -> sample_add_noise -> text pass -> UNet forward, shared by the train step and the held-out
        evaluation.  cached: the moments come out of the moment cache (no encoder launches); write_cache: the encoder's
        moments are stored at the batch's image slots.  noise_offset: the train step passes its option; the evaluation
        passes none whatever the engine was built with, so its launches and its numbers do not depend on the objective."""
        B, Lc, hw = self.B, self.cfg.vae.latent_channels, self.h * self.w
        # fork (overlap=True): the 16 mapper+CLIP passes (many small launches) run beside the VAE encoder (few large ones) on
        # a second stream; each schedule owns its split-K scratch, so they never alias.  OFF by default since round 6: both
        # sides fill the chip, and the two cross-stream edges of the captured graph cost more than the overlap returns
        # (same box, alternating processes: 39.96 / 39.98 / 40.05 steps/s without the fork, 39.08 / 39.75 / 39.79 with it;
        # profiles/r06_halo_persist_ab.txt) — the step is ONE linear chain of launches
        if fork:
            main = torch.cuda.current_stream()
            self.side.wait_stream(main)
            with torch.cuda.stream(self.side):
                self.text.forward()
                self.unet.forward_pre()  # time embedding + the 32 context K/V projections
        if cached:
            torch.index_select(self.mcache, 0, self.img_idx, out=self.vae.moments.view(B, hw, 2 * Lc))
        else:
            self.vae.forward()
            if write_cache:
                self.mcache.index_copy_(0, self.img_idx, self.vae.moments.view(B, hw, 2 * Lc))
        noise_args = (self.vae.moments, self.eps, self.noise, self.timesteps, self.ac, self.cfg.vae.scaling_factor,
                      self.cfg.ddpm.prediction_type == "v_prediction", self.latents, self.unet.x_in, self.target, B, Lc, hw)
        if noise_offset is None:
            ops.sample_add_noise(*noise_args)
        else:
            ops.sample_add_noise_offset(*noise_args, self.offset_noise, noise_offset)
        if fork:
            main.wait_stream(self.side)  # join
        else:
            self.text.forward()
            self.unet.forward_pre()
        self.unet.forward_main()

    def _grad_norm(self):
        """sum of squares of the object side (the whole object range, or the active segment of several) and of the view
        side, then one finish launch: norms, finite flag and clip coefficient into norm_out, and the optimizer's part of
        the ring row of the micro-step that closed the group.  After all_reduce(): every rank computes the same norm."""
        no = self.n_all_obj
        if self.n_objects > 1:
            ops.grad_sumsq(self.grads[:no], self.norm_ws_obj, seg_len=self.n_obj, active=self.obj_slot)
        else:
            ops.grad_sumsq(self.grads[:no], self.norm_ws_obj)
        if self._n_ws_view:
            ops.grad_sumsq(self.grads[no:], self.norm_ws_view)
        ops.grad_norm_finish(self.norm_ws_obj, self._n_ws_obj, self.norm_ws_view, self._n_ws_view, self.scaler, self.hyper,
                             self.max_norm_dev, self.norm_out, self.tele_ring, self.tele_count, self.telemetry_rows,
                             ops.telemetry_row_floats(self.B) if self.telemetry_rows else 0)

    def optimizer_step(self):
        self._refuse_ema_weights("optimizer_step()")
        self._adamw()
        if self.ema is not None:
            # after the call that carried OPT_FINISH: opt_step has advanced iff the step was applied.  One flat launch over
            # the whole bucket, one count (EMAModel over all parameters); a mapper that never trained has p == ema exactly
            ops.ema_update(self.ema, self.params, self.opt_step, self.ema_count, self.ema_hyper, self.ema_coef)

    def _adamw(self):
        a = (self.hyper, self.scaler, self.opt_step)
        kw = dict(growth_interval=self.growth_interval)
        flat, segments = ops.adamw_flat, ops.adamw_segments
        if self._norm_path:
            self._grad_norm()
        if self.max_grad_norm is not None:
            # the same calls in the same CHECK / APPLY / FINISH order, gradient times the clip coefficient (a device scalar)
            a += (self.norm_out[ops.NORM_CLIP_COEF:],)
            flat, segments = ops.adamw_flat_clipped, ops.adamw_segments_clipped
        if self.n_objects == 1:
            flat(self.params, self.grads, self.exp_avg, self.exp_avg_sq, *a, **kw)
            return
        # several buckets, one optimizer step: check all, apply all, then GradScaler.update once
        no = self.n_all_obj
        obj = (self.params[:no], self.grads[:no], self.exp_avg[:no], self.exp_avg_sq[:no], self.n_obj, self.n_objects,
               self.seg_step, self.obj_slot)
        view = (self.params[no:], self.grads[no:], self.exp_avg[no:], self.exp_avg_sq[no:])
        has_view = self.params.numel() > no
        if has_view:
            flat(*view, *a, phases=ops.OPT_CHECK, **kw)
        segments(*obj, *a, phases=ops.OPT_CHECK, **kw)
        if has_view:
            flat(*view, *a, phases=ops.OPT_APPLY, **kw)
        segments(*obj, *a, phases=ops.OPT_APPLY | ops.OPT_FINISH, **kw)

    # ------------------------------------------------------------------ the averaged mappers
    def _refuse_ema_weights(self, what: str):
        if self._ema_swapped:
            raise RuntimeError(f"{what} inside ema_weights(): `params` holds the average; leave the context first")

    def ema_weights(self):
        """context manager: `params` holds the EMA (and `ema` the raw weights) while it is open — one swap_f32 launch on
        enter, one on exit, both bit copies — so eval_losses(), an InferenceEngine over the live bucket and mapper saving
        see the average through the code path they always use.  Legal between optimizer steps only; training, capture and
        the state calls raise inside it."""
        from contextlib import contextmanager
        if self.ema is None:
            raise RuntimeError("ema_weights(): this engine was built without ema_decay")
        self._refuse_ema_weights("ema_weights()")
        if self.micro != 0:
            raise RuntimeError(f"ema_weights() inside a gradient-accumulation group (micro-step {self.micro} of "
                               f"{self.grad_accum}): legal between optimizer steps only")

        @contextmanager
        def swapped():
            ops.swap_f32(self.params, self.ema)
            self._ema_swapped = True
            try:
                yield self
            finally:
                ops.swap_f32(self.params, self.ema)
                self._ema_swapped = False

        return swapped()

    # ------------------------------------------------------------------ per-step record
    def read_telemetry(self):
        """the micro-steps recorded since the last read, oldest first: (rows, lost).  One device -> host copy and sync.  A
        row is a dict {micro_step, micro, timesteps[B], losses[B], closed}; the row of the micro-step that closed an
        accumulation group also has skipped, clip_coef, loss_scale, lr and grad_norm {total, object?, view?}.  lost: the
        micro-steps the ring had already overwritten (more than telemetry_rows since the last read)."""
        if not self.telemetry_rows:
            raise RuntimeError("read_telemetry(): this engine was built with telemetry_rows=0")
        from .telemetry import decode_ring
        host = self.tele_buf.cpu()
        count = int(host[0])
        ring = host[4:].view(torch.float32).view(self.telemetry_rows, -1)
        rows, lost = decode_ring(ring, count, min(self._tele_read, count), self.B)
        self._tele_read = count
        self.telemetry_lost += lost
        return rows, lost

    # ------------------------------------------------------------------ held-out evaluation
    def eval_forward(self):
        """the forward half of the step on the batch of set_batch(..., for_eval=True) and the randomness of set_noise(): VAE
        encoder -> sample_add_noise -> text pass in eval mode (no nested-dropout draw) -> UNet -> one MSE per sample into
        eval_out.  A strict subset of forward_backward's launches plus the per-sample loss: it reads the trainable state and
        writes activations only — no RNG advance, no loss_sum, no gradient, no optimizer, no moment-cache write."""
        B, Lc, hw = self.B, self.cfg.vae.latent_channels, self.h * self.w
        mode = self.text.training
        self.text.training = False
        try:
            self._forward_half(cached=False, write_cache=False)
            ops.mse_loss_per_sample(self.unet.pred, self.target, self.eval_out, self.eval_ws, B, Lc, hw)
        finally:
            self.text.training = mode

    def eval_losses(self, graph: bool = True, weights: Optional[torch.Tensor] = None):
        """per-sample diffusion losses of the current batch, CPU float32 [B] (forces a device sync).  Legal between
        optimizer steps only.  graph=True replays `graph_eval`, captured on first use (and again by capture());
        graph=False launches eagerly.  They are unmasked whatever the engine was built with.
        weights: f32 device [B][h*w] (rows of vneti_loss_weights_from_mask, e.g. `loss_weights`): returns the pair
        (unmasked, masked); the masked ones are one more per-sample launch behind the same forward."""
        if self.micro != 0:
            raise ValueError(f"eval_losses() inside a gradient-accumulation group (micro-step {self.micro} of "
                             f"{self.grad_accum}): legal between optimizer steps only")
        if weights is not None:
            if tuple(weights.shape) != (self.B, self.h * self.w) or weights.dtype != torch.float32 or not weights.is_cuda \
                    or not weights.is_contiguous():
                raise ValueError(f"eval_losses(): weights must be a contiguous f32 device tensor {(self.B, self.h * self.w)}")
            if self.eval_out_masked is None:
                self.eval_out_masked = torch.zeros_like(self.eval_out)
        if not graph:
            self.eval_forward()
        else:
            if self.graph_eval is None:
                self._capture_eval()
            self.graph_eval.replay()
        if weights is None:
            return self.eval_out.cpu()
        # (outside the captured evaluation: the graph, its launches and its numbers do not know about the mask)
        B, Lc, hw = self.B, self.cfg.vae.latent_channels, self.h * self.w
        ops.mse_loss_per_sample_weighted(self.unet.pred, self.target, weights, self.eval_out_masked, self.eval_ws, B, Lc, hw)
        return self.eval_out.cpu(), self.eval_out_masked.cpu()

    def _capture_eval(self):
        """the warm-up launch is an evaluation itself: nothing to snapshot"""
        self.graph_eval = capture_graphs([self.eval_forward], warmup=self.eval_forward)[0]

    def all_reduce(self):
        """the one exchange step of data-parallel training: sum the mapper gradients over ranks
        (the 1/world_size is folded into AdamW).  With several object mappers every rank trains the
        same scene per step (same scene-sampler seed), so only that segment and the view mapper move."""
        if self.world_size > 1:
            from ..parallel import all_reduce_plan_, reduce_plan
            plan = reduce_plan(self.n_obj, self.n_objects, self.active_object, self.grads.numel())
            if len(plan) > 1 and self._reduce_stage is None:  # scene segment + view mapper, packed
                self._reduce_stage = torch.empty(sum(b - a for a, b in plan), dtype=self.grads.dtype, device=self.grads.device)
            self.last_reduce_bytes = all_reduce_plan_(self.grads, plan, self._reduce_stage, comm=self.exchange)

    def _exchange_capturable(self) -> bool:
        """the all-reduce may sit INSIDE a graph: a stream-ordered library communicator, and a plan that does not depend on
        host state (several object mappers pack the active scene's segment, chosen per step on the host)"""
        return self.world_size > 1 and self.exchange is not None and self.n_objects == 1

    def _use_cache(self) -> bool:
        """decided on the host per micro-batch: does the batch consist of cached images only"""
        return bool(self.n_cache) and self._batch_cached

    def _mark_cached(self, used_cache: bool):
        """after the micro-step is enqueued: a batch that ran the encoder has its images' moments in the cache (stream order
        makes them visible to every later step).  Marking BEFORE the launch would leave stale slots behind a step that
        failed to enqueue."""
        if self.n_cache and not used_cache:
            self._cached_images.update(self._batch_images)
            self._batch_cached = bool(self._batch_images)  # the same batch again is served from the cache

    def reset_moment_cache(self, image_idx=None):
        """forget cached moments: all of them, or the listed dataset indices — for callers whose pixels behind an index
        change (the cache is only as deterministic as the dataset the CALLER vouched for)"""
        if not self.n_cache:
            return
        if image_idx is None:
            self._cached_images.clear()
        else:
            self._cached_images.difference_update(int(i) for i in image_idx)
        self._batch_cached = all(i in self._cached_images for i in self._batch_images) and bool(self._batch_images)

    def _refuse_eval_batch(self):
        if self._eval_batch:
            raise RuntimeError("the current batch was set with for_eval=True (held-out evaluation): call set_batch() with a "
                               "training batch before step()")

    def step_eager(self):
        """one micro-step; the optimizer runs after every `grad_accum`-th micro-step."""
        self._refuse_ema_weights("step()")
        self._refuse_eval_batch()
        cached = self._use_cache()
        self.forward_backward(accumulate=self.micro > 0, cached=cached)
        self._mark_cached(cached)
        self.micro += 1
        if self.micro == self.grad_accum:
            self.micro = 0
            self.all_reduce()
            self.optimizer_step()
            return True
        return False

    # ------------------------------------------------------------------ hipGraph capture
    def capture(self):
        """Capture the step into ONE hipGraph: forward + backward, (world > 1 on RCCL: the all-reduce of the flat gradient
        bucket as one collective node,) fused AdamW — the launch list of N GPUs is the one-GPU list plus that node.
        Fallbacks keep the older shape [forward+backward] -> host-issued all-reduce -> [optimizer]: the gloo backend,
        several object mappers (host-dependent exchange plan), and a communicator that refuses capture."""
        import os
        self._refuse_ema_weights("capture()")
        want = self._exchange_capturable()
        err = None
        try:
            self._capture(want)
        except RuntimeError as e:
            if not want:
                raise
            err = e
        if not want:
            return
        # the route is a COLLECTIVE decision: one rank replaying [graph A -> host all-reduce on torch's communicator ->
        # graph B] beside ranks whose collective sits in their graph on the library's communicator would never pair up
        from ..parallel import all_agree
        if all_agree(err is None):
            return
        if os.environ.get("VNETI_REQUIRE_ONE_GRAPH", "0") == "1":
            raise RuntimeError("VNETI_REQUIRE_ONE_GRAPH=1: the RCCL all-reduce could not be captured into the step's graph "
                               f"on {'this' if err else 'another'} rank" + (f" ({err})" if err else ""))
        import warnings
        warnings.warn(f"capturing the RCCL all-reduce failed on {'this' if err else 'another'} rank"
                      + (f" ({err})" if err else "") + "; every rank runs the exchange between two graphs")
        torch.cuda.synchronize()
        self.graph_a = self.graph_b = self.graph_acc = self.graph_a_c = self.graph_acc_c = None
        self._capture(False)

    def _capture(self, exchange_in_graph: bool):
        # the warm-up launches below are real steps: snapshot the trainable / RNG state and put it back — ALSO when the
        # capture raises (the fallback re-captures from the same state, not from one optimizer step later)
        # (and the record's ring, its counter and the norm outputs: the warm-up must leave no rows behind)
        saved = (self.params, self.exp_avg, self.exp_avg_sq, self.opt_step, self.scaler, self.rng_state, self.seg_step,
                 *self._ephemeral, *((self.ema, self.ema_count) if self.ema is not None else ()))
        state = [t.clone() for t in saved]
        try:
            self._capture_graphs(exchange_in_graph)
        finally:
            torch.cuda.synchronize()
            for dst, src in zip(saved, state):
                dst.copy_(src)
            self.micro = 0

    def _capture_graphs(self, exchange_in_graph: bool):
        fused_opt = (self.world_size == 1 or exchange_in_graph) and self.grad_accum == 1
        self.exchange_in_graph = exchange_in_graph

        def micro_step(accumulate, cached):
            self.forward_backward(accumulate=accumulate, cached=cached)
            if fused_opt:  # (only without accumulation)
                self.all_reduce()  # no-op at world 1; one captured collective node otherwise
                self.optimizer_step()

        def exchange_and_optimizer():
            if exchange_in_graph:
                self.all_reduce()
            self.optimizer_step()

        # capture order: a, acc, a_c, acc_c, b.  The _c graphs are the same steps with the moments read from the cache
        # instead of the encoder
        names = {(False, False): "graph_a", (True, False): "graph_acc", (False, True): "graph_a_c", (True, True): "graph_acc_c"}
        plan = [(names[acc, cached], partial(micro_step, acc, cached))
                for cached in ((False, True) if self.n_cache else (False,))
                for acc in ((False, True) if self.grad_accum > 1 else (False,))]
        if not fused_opt:
            plan.append(("graph_b", exchange_and_optimizer))

        def warmup():  # real steps on the capture stream (also primes RCCL): _capture() restores the state
            for _ in range(self.grad_accum):
                self.step_eager()

        for (name, _), graph in zip(plan, capture_graphs([body for _, body in plan], warmup)):
            setattr(self, name, graph)
        if self.graph_eval is not None:  # captured before this (re-)capture: renew it with the others
            self.graph_eval = None
            self._capture_eval()

    def step(self) -> bool:
        """one micro-step (graph replay when captured); returns True when the optimizer stepped."""
        if self.graph_a is None:
            return self.step_eager()
        self._refuse_ema_weights("step()")
        self._refuse_eval_batch()
        if self.exchange_in_graph and getattr(self.exchange, "closed", False):
            raise RuntimeError("the step's graph holds a collective on an RCCL communicator that has been closed (process "
                               "group re-initialised?): rebuild the engine")
        cached = self._use_cache()
        if cached:
            (self.graph_a_c if self.micro == 0 else self.graph_acc_c).replay()
        else:
            (self.graph_a if self.micro == 0 else self.graph_acc).replay()
        self._mark_cached(cached)
        self.micro += 1
        if self.micro < self.grad_accum:
            return False
        self.micro = 0
        if self.graph_b is not None:
            if not self.exchange_in_graph:
                self.all_reduce()
            self.graph_b.replay()
        if self.exchange_in_graph:
            from .. import parallel
            parallel.COLLECTIVE_CALLS += 1  # the replayed collective node
        return True

    def loss(self) -> float:
        """the training loss of the last step: the mean squared error, Min-SNR weighted when snr_gamma is set — the quantity
        being minimised (forces a device sync — call sparingly)."""
        return float(self.loss_sum.item()) / self.n_loss

    # ------------------------------------------------------------------ introspection
    def launches(self) -> List:
        out = list(self.vae.fwd) + list(self.text.fwd) + list(self.unet.fwd_pre) + list(self.unet.fwd)
        if self.need_backward:
            out += list(self.unet.bwd) + list(self.text.bwd)
        return out

    def memory_bytes(self) -> int:
        own = 0 if self.loss_weights is None else self.loss_weights.numel() * 4 + self._mask_ws.numel() * 4
        return self.unet.bytes + self.vae.bytes + self.text.bytes + own
