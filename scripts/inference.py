"""Generate images with the mappers of a run.  Two command lines:

  * the reference's DTU novel-view evaluation (its scripts/inference.py contract, `InferenceConfig`): every evaluation
    view x seed (x evaluation object in mode 3), batched (`batch` prompts per sampler run), written to
    `inference_dir` as preds_object_{tok}_iter_{it}_seed{s}.png and results_all_iter_{it}_scans_{toks}_seeds_{seeds}.pt

    python scripts/inference.py --config_path input_configs/inference.yaml --input_dir <run> --iteration 1500 \
        [--seeds [0,1]] [--batch 8] [--do_lpips true --lpips_vgg_weights A.pth --lpips_lin_weights B.pth] \
        [--use_ema true]   (the averaged mappers mapper-ema-steps-N_* of a run with optim.ema_decay; missing files raise)
        [--guidance_rescale 0.7 --timestep_spacing trailing]   (Lin et al. 2023, for v-prediction models; off by default)

  * free prompts x seeds -> PNG files:

    python scripts/inference.py --exp_dir results/train --prompt "<view_dtu12d_cam22_…>. A photo of a <object>" \
        --seeds 0 1 --steps 30 --guidance 7.5 --out out/ [--guidance_rescale 0.7 --timestep_spacing trailing]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from view_neti_amd.compat.inference import load_inference  # noqa: E402
from view_neti_amd.compat.sd_pipeline_call import sd_pipeline_call  # noqa: E402


REFERENCE_KEYS = ("--config_path", "--input_dir", "--iteration")


def main_reference(args):
    from view_neti_amd.compat.inference_dtu import parse_inference_config, run
    results = run(parse_inference_config(args))
    for key, res in results.items():
        print(key, {k: round(v, 5) for k, v in res.items() if k.endswith("_mean")})


def main():
    if any(a.split("=")[0] in REFERENCE_KEYS for a in sys.argv[1:]):
        return main_reference(sys.argv[1:])
    ap = argparse.ArgumentParser()
    ap.add_argument("--exp_dir", required=True)
    ap.add_argument("--mapper", default="mapper-final")
    ap.add_argument("--prompt", action="append", required=True)
    ap.add_argument("--seeds", type=int, nargs="+", default=[0])
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--guidance", type=float, default=7.5)
    ap.add_argument("--sampler", default="dpm++2m", choices=["dpm++2m", "ddim"])
    ap.add_argument("--truncation_idx", type=int, default=None)
    ap.add_argument("--guidance_rescale", type=float, default=0.0, help="diffusers' guidance_rescale in [0, 1]; 0: off")
    ap.add_argument("--timestep_spacing", default=None, choices=["trailing"], help="default: the scheduler's own list")
    ap.add_argument("--out", default="inference_out")
    a = ap.parse_args()
    pipe, pm = load_inference(a.exp_dir, a.mapper, batch=1, sampler=a.sampler)
    pipe.timestep_spacing = a.timestep_spacing
    os.makedirs(a.out, exist_ok=True)
    for pi, prompt in enumerate(a.prompt):
        emb = pm.embed_prompt(prompt, truncation_idx=a.truncation_idx)
        for seed in a.seeds:
            out = sd_pipeline_call(pipe, emb, num_inference_steps=a.steps, guidance_scale=a.guidance,
                                   generator=torch.Generator().manual_seed(seed), guidance_rescale=a.guidance_rescale)
            path = os.path.join(a.out, f"p{pi}_s{seed}.png")
            out.images[0].save(path)
            print(path)


if __name__ == "__main__":
    main()
