"""Dev tool: batched DTU novel-view evaluation throughput.  Synthetic SD-2.1 shapes, DPM-Solver++ 30 steps + CFG, one
evaluation = 34 views x 2 seeds (distinct view tokens, per-sample seeds; the views alternate between two objects'
mappers, so the per-sample object slots are exercised), rendered in batches of B with the last batch padded, as
compat/inference_dtu.py does.  The B arms are built once and timed in alternation, `--repeats` rounds, on the same
box.  Prints one JSON line per resolution."""
import os
os.environ.setdefault("VNETI_ALLOW_SYNTHETIC_WEIGHTS", "1")  # dev tool: synthetic SD-shaped weights on purpose
import argparse, json, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from view_neti_amd import ops, sd_config as sc, synth
from view_neti_amd.compat.inference_dtu import plan_batches
from view_neti_amd.engine.infer import InferenceEngine
from view_neti_amd.engine.text import flatten_mapper_state
from view_neti_amd.mapper import fourier_frequencies, init_mapper_state

ap = argparse.ArgumentParser()
ap.add_argument("--model", default="sd21")
ap.add_argument("--sizes", default="768x576,768x768", help="WxH list")
ap.add_argument("--batches", default="1,4,8")
ap.add_argument("--steps", type=int, default=30)
ap.add_argument("--views", type=int, default=34)
ap.add_argument("--seeds", type=int, default=2)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--guidance_rescale", type=float, default=0.0, help="diffusers' guidance_rescale (0: off)")
ap.add_argument("--timestep_spacing", default=None, choices=["trailing"])
a = ap.parse_args()
cfg = sc.CONFIGS[a.model]()
dev = "cuda"
uw, dw, cw = (synth.unet_weights(cfg.unet, device=dev), synth.vae_decoder_weights(cfg.vae, device=dev),
              synth.clip_weights(cfg.clip, device=dev))
D, V = cfg.clip.hidden_size, cfg.clip.vocab_size
torch.manual_seed(0)
w_enc = fourier_frequencies([0.03, 2.0], 64, 0)
w_enc_v = fourier_frequencies([0.03, 2.0] + [0.5] * 12, 64, 0)
objs = [init_mapper_state(64, 64, D), init_mapper_state(64, 64, D)]
sdv = init_mapper_state(64, 64, D)
n_each = ops.mapper_num_params(64, 64, D, True)
stride = (n_each + 3) // 4 * 4
bucket = torch.zeros(2 * stride)
for k, sd in enumerate(objs):
    bucket[k * stride:k * stride + n_each] = flatten_mapper_state(sd)
bucket = bucket.to(dev)
norm = float(cw["text_model.embeddings.token_embedding.weight"][:1000].float().norm(dim=1).mean())
obj_ids = [V - 3, V - 100]
view_ids = [V - 4 - c for c in range(a.views)]
vparams = synth.gaussian((a.views, 12), 9).clamp(-1, 1)
neg = synth.input_ids(1, obj_ids[0], V)
neg[neg == obj_ids[0]] = 7


def evaluation(eng, B):
    n_img = 0
    for plan, n in plan_batches([None], list(range(a.views)), list(range(a.seeds)), B):
        entries = [(c % 2, c, s) for _, c, s in plan]  # (object, view, seed)
        ids = torch.cat([synth.input_ids(1, obj_ids[o], V, view_placeholder_id=view_ids[c]) for o, c, _ in entries])
        eng.set_prompts(ids, torch.tensor([obj_ids[o] for o, _, _ in entries]),
                        torch.tensor([view_ids[c] for _, c, _ in entries]),
                        torch.stack([vparams[c] for _, c, _ in entries]), slots=[o for o, _, _ in entries])
        lat = torch.cat([torch.randn((1, 4, eng.h, eng.w), generator=torch.Generator().manual_seed(s))
                         for _, _, s in entries])
        img = eng.generate(lat, a.steps, 7.5, "dpm++2m", guidance_rescale=a.guidance_rescale,
                           timestep_spacing=a.timestep_spacing)
        img[:n].cpu()  # what the driver does with each batch: the real entries go to the host
        n_img += n
    return n_img


for size in a.sizes.split(","):
    W, H = (int(v) for v in size.split("x"))
    engines = {}
    for B in (int(b) for b in a.batches.split(",")):
        t0 = time.time()
        eng = InferenceEngine(cfg, uw, dw, cw, B, H, W, None, w_enc, norm, 5.0, mapper_view=sdv, w_enc_view=w_enc_v,
                              norm_scale_view=norm, alpha_view=5.0, params_object=bucket, object_slot_stride=stride,
                              per_sample_slots=True)
        eng.set_negative_prompt(neg)
        evaluation(eng, B)  # warm-up: graph capture, autotune caches
        torch.cuda.synchronize()
        engines[B] = (eng, time.time() - t0)
    times = {B: [] for B in engines}
    for r in range(a.repeats):
        order = list(engines) if r % 2 == 0 else list(reversed(engines))  # arms alternated
        for B in order:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            n_img = evaluation(engines[B][0], B)
            torch.cuda.synchronize()
            times[B].append(time.perf_counter() - t0)
    base = statistics.median(times[min(times)])
    out = {"metric": f"NVS evaluation images/s ({a.model} {W}x{H}, dpm++2m-{a.steps}, CFG, {a.views * a.seeds} "
                     f"images = {a.views} views x {a.seeds} seeds)", "unit": "images/s",
           "guidance_rescale": a.guidance_rescale, "timestep_spacing": a.timestep_spacing, "arms": {}}
    for B, ts in times.items():
        med = statistics.median(ts)
        out["arms"][f"B{B}"] = {"images_per_s": n_img / med, "s_per_image": med / n_img, "speedup_vs_B1": base / med,
                                "runs_s": [round(t, 3) for t in ts], "decode_batch": engines[B][0].decode_batch,
                                "build_s": round(engines[B][1], 1)}
    print(json.dumps(out), flush=True)
    del engines
    torch.cuda.empty_cache()
