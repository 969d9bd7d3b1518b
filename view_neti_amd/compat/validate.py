"""Validation images during training — the trigger and file naming of the reference's `ValidationHandler`
(training/validate.py, called from coach.py:243-251 when `global_step % eval.validation_steps == 0`), without its
DTU metric harness (masked MSE/PSNR/SSIM/LPIPS against ground-truth views needs the DTU masks and LPIPS weights:
SURVEY §8 f4, out of scope).

What is produced, with the live mapper parameters (the inference engine aliases the trainer's parameter bucket):
  * learnable_mode 0: every `eval.validation_prompts` template filled with the object token x `eval.validation_seeds`
    -> one grid per prompt, `validation-iter_{step}-…_imgs_t2i_{i}.png` (validate.py:296-309);
  * view modes: "<view token>. A photo of a <object>" for the training views x seeds -> the camidx -> images dict the
    reference saves (`validation-iter_{step}-denoisesteps_{N}_numseeds_{k}_upsample_{u}.pt`, validate.py:111-118)
    and a grid PNG per seed.
  * view modes with `eval.validation_nvs` (extension switch, off by default): what the reference's
    handler does (validate.py:65-186) — the 34 evaluation views of `get_cam_idxs(dtu_subset)` x seeds (x evaluation
    objects) at the novel-view resolution, `eval.validation_nvs_batch` prompts per sampler run through
    `inference_dtu.generate_views`, the same `.pt` (camidx -> uint8 (n_seeds, H, W, 3)), scored against the scene with
    `inference_dtu.evaluate`: one grid / figure per seed under the same `…_seed_{seed}.png` names and `…_metrics.json`.
"""
from __future__ import annotations

from pathlib import Path
from typing import List

import numpy as np
import torch
from PIL import Image

from ..engine.infer import InferenceEngine
from .prompt_manager import PromptManager
from .sd_pipeline_call import InferencePipeline, sd_pipeline_call


def make_grid(images: List[np.ndarray], nrow: int) -> Image.Image:
    """uint8 HWC images -> one image, row-major, `nrow` per row (torchvision.utils.make_grid without padding)."""
    h, w = images[0].shape[:2]
    rows = (len(images) + nrow - 1) // nrow
    canvas = np.zeros((rows * h, nrow * w, 3), dtype=np.uint8)
    for i, im in enumerate(images):
        r, c = divmod(i, nrow)
        canvas[r * h:(r + 1) * h, c * w:(c + 1) * w] = im
    return Image.fromarray(canvas)


class ValidationHandler:
    def __init__(self, coach, unet_w, vae_dec_w, clip_w):
        self.coach = coach
        self.cfg = cfg = coach.cfg
        eng = coach.engine
        m = cfg.model
        # learnable_mode 1 trains no object mapper (the object is a vocabulary word, dataset.py:654-668): the engine's object
        # side is the Coach's stand-in, which no prompt reaches (placeholder -1)
        first = coach._standin_object if cfg.learnable_mode == 1 else \
            coach.mapper_object_lookup[coach.placeholder_object_token_ids[0]]
        self.nvs = bool(cfg.eval.validation_nvs)
        if self.nvs:
            self._init_nvs(first, unet_w, vae_dec_w, clip_w)
            return
        h, w = coach._image_hw()
        kw = {}
        if coach.mapper_view is not None:
            mv = coach.mapper_view
            frozen = eng.view_params_flat().numel() == 0  # modes 4/5 train no view mapper: it is not in the bucket
            kw = dict(w_enc_view=mv.encoder.w, norm_scale_view=mv.norm_scale, alpha_view=m.output_bypass_alpha_view,
                      unconstrained_view=m.bypass_unconstrained_view, output_bypass_view=mv.output_bypass,
                      **(dict(mapper_view=mv.mapper_state()) if frozen else dict(params_view=eng.view_params_flat())))
        self.slot = torch.zeros(1, dtype=torch.int32, device=eng.dev)
        self.engine = InferenceEngine(
            coach.sd, unet_w, vae_dec_w, clip_w, 1, h, w, None, first.encoder.w, first.norm_scale,
            m.output_bypass_alpha_object, hidden_object=first.hidden, unconstrained_object=m.bypass_unconstrained_object,
            device=eng.dev, params_object=eng.params[: eng.n_all_obj], object_slot=self.slot,
            object_slot_stride=eng.n_obj, **first.engine_encoder_kwargs(), **kw)
        self.pipeline = InferencePipeline(self.engine, coach.tokenizer, "dpm++2m",
                                          timestep_spacing=self.cfg.eval.timestep_spacing)
        self.prompt_manager = PromptManager(
            coach.tokenizer, placeholder_view_token_ids=coach.placeholder_view_token_ids,
            placeholder_object_token_ids=coach.placeholder_object_token_ids,
            view_params_fn=lambda tid: coach._view_params(torch.tensor([tid]))[0])

    def _view_kwargs(self):
        """the view side of the validator's engine: the trainer's live bucket, or the frozen mapper of modes 4 / 5"""
        coach, m = self.coach, self.cfg.model
        if coach.mapper_view is None:
            return {}
        mv, eng = coach.mapper_view, coach.engine
        frozen = eng.view_params_flat().numel() == 0
        return dict(w_enc_view=mv.encoder.w, norm_scale_view=mv.norm_scale, alpha_view=m.output_bypass_alpha_view,
                    unconstrained_view=m.bypass_unconstrained_view, output_bypass_view=mv.output_bypass,
                    **(dict(mapper_view=mv.mapper_state()) if frozen else dict(params_view=eng.view_params_flat())))

    def _init_nvs(self, first, unet_w, vae_dec_w, clip_w):
        """eval.validation_nvs: a batched per-sample-slot engine at the novel-view resolution over the trainer's live bucket.
        Held-out cameras have no token in the run's tokenizer (it holds the training views), so the prompts go through a
        tokenizer of their own with all 49 view tokens, as compat/inference.py builds it; the engine reads camera
        parameters and mapper slots, never these ids' embedding rows, which exist only so that the table covers them."""
        from . import inference_dtu as nvs
        from .dtu_metrics import get_cam_idxs
        from .tokenizer import load_tokenizer
        coach, cfg = self.coach, self.cfg
        eng, ds, m, ev = coach.engine, coach.train_dataset, cfg.model, cfg.eval
        if cfg.learnable_mode == 0 or cfg.data.camera_representation != "dtu-12d":
            raise ValueError("eval.validation_nvs renders the DTU evaluation views: it needs a view mode (learnable_mode 1-5) "
                             "on camera_representation dtu-12d")
        h, w = nvs.nvs_resolution(cfg, coach.sd)
        tok = load_tokenizer(str(m.pretrained_model_name_or_path), coach.sd.clip.vocab_size)
        lut = ds.lookup_camidx_to_view_token
        view_tokens = [lut[k] for k in sorted(lut)]
        object_tokens = list(ds.placeholder_object_tokens)
        tok.add_tokens(view_tokens + object_tokens)
        view_ids = tok.convert_tokens_to_ids(view_tokens)
        object_ids = tok.convert_tokens_to_ids(object_tokens) if object_tokens else []
        key = "text_model.embeddings.token_embedding.weight"
        E = clip_w[key]
        if len(tok) > E.shape[0]:
            clip_w = dict(clip_w)
            clip_w[key] = torch.cat([E, E[coach.super_object_id].unsqueeze(0).repeat(len(tok) - E.shape[0], 1)], 0)
        self.engine = InferenceEngine(
            coach.sd, unet_w, vae_dec_w, clip_w, ev.validation_nvs_batch, h, w, None, first.encoder.w, first.norm_scale,
            m.output_bypass_alpha_object, hidden_object=first.hidden, unconstrained_object=m.bypass_unconstrained_object,
            device=eng.dev, params_object=eng.params[: eng.n_all_obj], object_slot_stride=eng.n_obj, per_sample_slots=True,
            **first.engine_encoder_kwargs(), **self._view_kwargs())
        # this tokenizer's object ids -> the trainer's slots (slot k = k-th placeholder object token, as in the Coach)
        self.pipeline = InferencePipeline(self.engine, tok, "dpm++2m", object_slot={tid: k for k, tid in enumerate(object_ids)},
                                          timestep_spacing=ev.timestep_spacing)
        self.pipeline.object_tokens = object_tokens
        id2tok = dict(zip(view_ids, view_tokens))
        mv = coach.mapper_view

        def cam_fn(token_id: int) -> torch.Tensor:  # Coach._view_params for any of the 49 cameras
            p = ds.dtu_token_to_cam_params(id2tok[token_id])[0]
            return (p - mv.cam_mins) / (mv.cam_maxs - mv.cam_mins) * 2 - 1

        self.prompt_manager = PromptManager(tok, placeholder_view_token_ids=view_ids,
                                            placeholder_object_token_ids=object_ids, view_params_fn=cam_fn)
        if cfg.learnable_mode == 3:
            self.nvs_keys = list(ev.eval_placeholder_object_tokens or object_tokens[:1])
        else:
            self.nvs_keys = [None]
        self.nvs_objects = [nvs.eval_object_token(cfg, object_tokens, k) for k in self.nvs_keys]
        self.nvs_cams, _, _ = get_cam_idxs(cfg.data.dtu_subset)
        # a missing ground-truth view stops the run now, not at the first validation step
        for k, obj in zip(self.nvs_keys, self.nvs_objects):
            scene, _ = nvs.scene_of(cfg, obj if cfg.learnable_mode == 3 else None)
            missing = [c for c in self.nvs_cams
                       if not (scene / ds.dtu_cam_and_lighting_to_fname(c, cfg.data.dtu_lighting)).is_file()]
            if missing:
                raise FileNotFoundError(f"eval.validation_nvs: {scene} lacks the ground-truth views of cameras {missing} "
                                        f"(lighting {cfg.data.dtu_lighting})")
        self.lpips_fn = None
        if ev.lpips_vgg_weights is not None and ev.lpips_lin_weights is not None:
            if cfg.optim.mixed_precision == "fp16":
                from .lpips import LPIPS
                self.lpips_fn = LPIPS.from_files(ev.lpips_vgg_weights, ev.lpips_lin_weights, device=eng.dev)
            else:
                coach.log("eval.validation_nvs: LPIPS skipped (it runs on the fp16 library only; this run is "
                          f"{cfg.optim.mixed_precision})")

    def _infer_nvs(self, step: int):
        import importlib.util
        import json
        from . import inference_dtu as nvs
        cfg, coach, ev = self.cfg, self.coach, self.cfg.eval
        exp = Path(cfg.log.exp_dir)
        seeds = list(ev.validation_seeds)
        stem = f"validation-iter_{step}-denoisesteps_{ev.num_denoising_steps}"
        base = f"{stem}_numseeds_{len(seeds)}_upsample_{ev.dtu_upsample_key}"
        preds = nvs.generate_views(self.pipeline, self.prompt_manager, self.nvs_objects, self.nvs_cams, seeds,
                                   ev.num_denoising_steps, guidance_rescale=ev.guidance_rescale)
        objs = self.nvs_objects
        torch.save(preds[objs[0]] if len(objs) == 1 else {o: preds[o] for o in objs}, exp / f"{base}.pt")
        figures = importlib.util.find_spec("matplotlib") is not None
        summary = {}
        for key, obj in zip(self.nvs_keys, objs):
            res = nvs.evaluate(cfg, preds[obj], seeds, obj if cfg.learnable_mode == 3 else None, make_figures=figures,
                               lpips_fn=self.lpips_fn)
            tag = "" if len(objs) == 1 else "_" + obj.strip("<>")
            for i, grid in enumerate(res["grids"]):
                name = exp / f"{base}{tag}_seed_{seeds[i]}.png"
                if res["figures"]:
                    res["figures"][i].savefig(name, dpi=300)
                    import matplotlib.pyplot as plt
                    plt.close(res["figures"][i])
                else:
                    Image.fromarray((grid.clamp(0, 1).numpy() * 255).round().astype(np.uint8)).save(name)
            summary[obj] = {k: v for k, v in res.items() if k.endswith("_mean")}
            coach.log(f"validation step {step} {obj}: " + "  ".join(f"{k} {v:.4f}" for k, v in summary[obj].items()))
        with open(exp / f"{stem}_metrics.json", "w") as f:
            json.dump(summary, f, indent=1)

    def _generate(self, prompt: str, seeds: List[int]) -> List[np.ndarray]:
        emb = self.prompt_manager.embed_prompt(prompt)
        tid = int(emb.input_ids_placeholder_object)
        self.slot.fill_(self.coach.object_slot.get(tid, 0))
        out = []
        for seed in seeds:
            img = sd_pipeline_call(self.pipeline, emb, num_inference_steps=self.cfg.eval.num_denoising_steps,
                                   generator=torch.Generator().manual_seed(seed), output_type="np",
                                   return_dict=False, guidance_rescale=self.cfg.eval.guidance_rescale)[0]
            out.append((img[0] * 255).round().astype(np.uint8))
        return out

    def infer(self, step: int):
        if self.nvs:
            return self._infer_nvs(step)
        cfg, coach = self.cfg, self.coach
        ev = cfg.eval
        exp = Path(cfg.log.exp_dir)
        stem = f"validation-iter_{step}-denoisesteps_{ev.num_denoising_steps}"
        seeds = list(ev.validation_seeds)
        if cfg.learnable_mode == 0:
            token = coach.train_dataset.placeholder_object_tokens[0]
            for i, tmpl in enumerate(ev.validation_prompts or []):
                imgs = self._generate(tmpl.format(token), seeds)
                make_grid(imgs, len(imgs)).save(exp / f"{stem}_upsample_{ev.dtu_upsample_key}_imgs_t2i_{i}.png")
            return
        ds = coach.train_dataset
        if cfg.learnable_mode == 1:
            tokens = [ds.fixed_object_token]  # validate.py:455: modes 1, 2, 4, 5 share the view-token prompts; here with the word
        else:
            tokens = (ev.eval_placeholder_object_tokens or ds.placeholder_object_tokens[:1]) if cfg.learnable_mode == 3 \
                else ds.placeholder_object_tokens[:1]
        result = {}
        for obj in tokens:
            per_cam = {}
            for view_token in ds.placeholder_view_tokens:
                cam = ds.lookup_view_token_to_camidx[view_token]
                per_cam[cam] = self._generate(f"{view_token}. A photo of a {obj}", seeds)
            result[obj] = per_cam
            for si, seed in enumerate(seeds):
                grid = make_grid([per_cam[c][si] for c in sorted(per_cam)], min(len(per_cam), 7))
                tag = "" if len(tokens) == 1 else "_" + obj.strip("<>")
                grid.save(exp / f"{stem}_numseeds_{len(seeds)}_upsample_{ev.dtu_upsample_key}{tag}_seed_{seed}.png")
        torch.save(result[tokens[0]] if len(tokens) == 1 else result,
                   exp / f"{stem}_numseeds_{len(seeds)}_upsample_{ev.dtu_upsample_key}.pt")
        if cfg.data.camera_representation == "dtu-12d":
            self._dtu_metrics(step, stem, result, seeds)

    def _dtu_metrics(self, step: int, stem: str, result, seeds):
        """validate.py:123-186: masked MSE / PSNR / SSIM of the generated views against the scene's ground truth
        (compat/dtu_metrics.py).  Runs when all the evaluation views of the split were generated at a 3:4 aspect and the
        ground-truth images are on disk; object masks default to all-white when the IDR masks are absent."""
        import json
        from . import dtu_metrics as dm
        cfg, coach = self.cfg, self.coach
        cam_idxs, _, _ = dm.get_cam_idxs(cfg.data.dtu_subset)
        summary = {}
        for obj, per_cam in result.items():
            if set(per_cam) != set(cam_idxs):
                continue
            h, w = per_cam[cam_idxs[0]][0].shape[:2]
            if h / w != 0.75:
                continue
            if cfg.learnable_mode == 3:
                scan_id = obj[5:-1]
                scene = Path(cfg.data.train_data_dir) / f"scan{scan_id}"
            else:
                scene, scan_id = Path(cfg.data.train_data_dir), Path(cfg.data.train_data_dir).stem[4:]
            if not scene.exists():
                continue
            pred = {c: np.stack(per_cam[c]) for c in cam_idxs}
            try:
                res = dm.evaluate_dtu_predictions(pred, scene, cfg.data.dtu_subset, cfg.data.dtu_lighting, 1, seeds,
                                                  scan_id=scan_id, make_figures=False)
            except FileNotFoundError:
                continue
            summary[obj] = {k: v for k, v in res.items() if k.endswith("_mean")}
            coach.log(f"validation step {step} {obj}: " + "  ".join(f"{k} {v:.4f}" for k, v in summary[obj].items()))
        if summary:
            with open(Path(cfg.log.exp_dir) / f"{stem}_metrics.json", "w") as f:
                json.dump(summary, f, indent=1)
