"""Cost of guidance rescale on the captured sampler step, in one process: BASELINE config 5 — SD-2.1 shapes,
768^2, DDIM-50, CFG 7.5, batch 1, synthetic weights — on one set of autotuner picks:

    off             guidance_rescale = 0: the sampler step as it always was
    rescale         guidance_rescale = 0.7 on the SAME engine: two factor launches more per step and the scaled step entry in
                    place of the step entry
    off (control)   a second build of the engine, guidance_rescale = 0: the resolution of the comparison

All are captured graphs.  The arms are timed in alternation, `--repeats` times; each window is one generation without the
decoder (ms per sampler step) and one with it (s per image), each ending in a device synchronise.  Also times the factor
entry alone with device events (launches back to back, outside the step).  Prints the windows, then one JSON line that says
whether the rescale arm's difference is inside the spread of the two off engines.  There is no pass bar: the comparison
is the off arm of the same run.

    python tools/bench_guidance_rescale.py [--model sd21] [--resolution 768] [--batch 1] [--steps 50] [--repeats 3]
"""
import os
os.environ.setdefault("VNETI_ALLOW_SYNTHETIC_WEIGHTS", "1")  # dev tool: synthetic SD-shaped weights on purpose
import argparse, json, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from view_neti_amd import ops, sd_config as sc, synth
from view_neti_amd.engine.infer import InferenceEngine
from view_neti_amd.mapper import fourier_frequencies, init_mapper_state

ap = argparse.ArgumentParser()
ap.add_argument("--model", default="sd21"); ap.add_argument("--resolution", type=int, default=768)
ap.add_argument("--batch", type=int, default=1); ap.add_argument("--steps", type=int, default=50)
ap.add_argument("--sampler", default="ddim"); ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--guidance_rescale", type=float, default=0.7)
ap.add_argument("--timestep_spacing", default=None, choices=["trailing"])
a = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("bench_guidance_rescale needs a GPU")
cfg = sc.CONFIGS[a.model]()
dev = "cuda"
uw, dw, cw = synth.unet_weights(cfg.unet, device=dev), synth.vae_decoder_weights(cfg.vae, device=dev), synth.clip_weights(cfg.clip, device=dev)
D = cfg.clip.hidden_size
torch.manual_seed(0)
w_enc = fourier_frequencies([0.03, 2.0], 64, 0); sdo = init_mapper_state(64, 64, D)
w_enc_v = fourier_frequencies([0.03, 2.0] + [0.5] * 12, 64, 0); sdv = init_mapper_state(64, 64, D)
norm = float(cw["text_model.embeddings.token_embedding.weight"][:1000].float().norm(dim=1).mean())
ph, phv = cfg.clip.vocab_size - 3, cfg.clip.vocab_size - 4
ids = synth.input_ids(a.batch, ph, cfg.clip.vocab_size, view_placeholder_id=phv)
neg = synth.input_ids(1, ph, cfg.clip.vocab_size); neg[neg == ph] = 7
lat = synth.gaussian((a.batch, 4, a.resolution // 8, a.resolution // 8), 17)


def build():
    t0 = time.time()
    eng = InferenceEngine(cfg, uw, dw, cw, a.batch, a.resolution, a.resolution, sdo, w_enc, norm, 5.0, mapper_view=sdv,
                          w_enc_view=w_enc_v, norm_scale_view=norm, alpha_view=5.0)
    eng.set_negative_prompt(neg)
    eng.set_prompt(ids, torch.full((a.batch,), ph), torch.full((a.batch,), phv), synth.gaussian((a.batch, 12), 9).clamp(-1, 1))
    return eng, time.time() - t0


def window(eng, phi, decode):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = eng.generate(lat, a.steps, 7.5, a.sampler, decode=decode, guidance_rescale=phi, timestep_spacing=a.timestep_spacing)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def factor_alone_us(eng, launches=200):
    """device time of one vneti_cfg_rescale_factor (partials + finish) on the engine's own buffers, back to back"""
    n = eng.h * eng.w
    call = lambda: ops.cfg_rescale_factor(eng.unet.pred, eng.rescale_factor, eng.rescale_ws, eng.B, eng.Lc, n, 7.5,
                                          a.guidance_rescale)
    for _ in range(10):
        call()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(launches):
        call()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) / launches * 1e3


first, build_first = build()
second, build_second = build()
del uw, dw, cw
arms = {"off": (first, 0.0), "rescale": (first, a.guidance_rescale), "off (control)": (second, 0.0)}
finite = {}
for name, (eng, phi) in arms.items():  # warm-up: graph capture, autotune caches
    _, img = window(eng, phi, True)
    finite[name] = bool(torch.isfinite(img).all())
assert len(first._graphs) == 2 and len(second._graphs) == 1
step_ms, image_s = {k: [] for k in arms}, {k: [] for k in arms}
for r in range(a.repeats):
    order = list(arms) if r % 2 == 0 else list(reversed(arms))  # arms alternated
    for name in order:
        eng, phi = arms[name]
        step_ms[name].append(window(eng, phi, False)[0] / a.steps * 1e3)
        image_s[name].append(window(eng, phi, True)[0] / a.batch)
    print(f"repeat {r}: " + "   ".join(f"{k} {step_ms[k][-1]:.3f} ms/step {image_s[k][-1]:.3f} s/image" for k in arms), flush=True)
med = lambda v: sorted(v)[len(v) // 2]
both_off = step_ms["off"] + step_ms["off (control)"]
spread_us = (max(both_off) - min(both_off)) * 1e3
diff_us = (med(step_ms["rescale"]) - med(step_ms["off"])) * 1e3
out = {"metric": f"guidance rescale on the captured sampler step ({a.model} {a.resolution}x{a.resolution}, {a.sampler}-{a.steps}, "
                 f"CFG 7.5, bs={a.batch})", "guidance_rescale": a.guidance_rescale, "timestep_spacing": a.timestep_spacing,
       "ms_per_sampler_step": {k: round(med(v), 4) for k, v in step_ms.items()},
       "ms_per_sampler_step_all": {k: [round(x, 4) for x in v] for k, v in step_ms.items()},
       "s_per_image": {k: round(med(v), 4) for k, v in image_s.items()},
       "s_per_image_all": {k: [round(x, 4) for x in v] for k, v in image_s.items()},
       "rescale_over_off_us_per_step": round(diff_us, 1),
       "control_over_off_us_per_step": round((med(step_ms["off (control)"]) - med(step_ms["off"])) * 1e3, 1),
       "off_spread_us_per_step": round(spread_us, 1),
       "difference_inside_control_spread": bool(abs(diff_us) <= spread_us),
       "factor_entry_alone_us": round(factor_alone_us(first), 2),
       "engine_gib": round(first.memory_bytes() / 2 ** 30, 3), "build_s": [round(build_first, 1), round(build_second, 1)],
       "image_finite": finite}
if out["difference_inside_control_spread"]:
    print(f"the rescale arm's difference ({diff_us:.1f} us per step) is INSIDE the spread of the two off engines "
          f"({spread_us:.1f} us): not resolved")
print(json.dumps(out))
