"""The three ways through the sampler — captured step replayed, eager loop, eager loop on conditioning handed in
(`generate_from_contexts`) — land on the same final latents bit for bit, for DDIM eta = 0, DDIM eta = 0.5 with one fixed
`step_noise`, and DPM-Solver++(2M); and the captured steps are cached per (guidance scale, noise term), not per call.
Tiny family, 64 x 64, B = 2, 3 steps, public API only: one engine serves every case of the file."""
import pytest
import torch

pytestmark = pytest.mark.gpu

B, H, W, STEPS, GS = 2, 64, 64, 3, 5.0
CASES = {"ddim": ("ddim", 0.0), "ddim_eta": ("ddim", 0.5), "dpm": ("dpm++2m", 0.0)}
_shared = {}


def _engine():
    if _shared:
        return _shared["eng"], _shared["lat"], _shared["noise"]
    from view_neti_amd import sd_config as sc, synth
    from view_neti_amd.engine.infer import InferenceEngine
    from view_neti_amd.mapper import fourier_frequencies, init_mapper_state
    cfg = sc.tiny()
    D = cfg.clip.hidden_size
    uw, dw, cw = synth.unet_weights(cfg.unet), synth.vae_decoder_weights(cfg.vae), synth.clip_weights(cfg.clip)
    gen = torch.Generator().manual_seed(9)
    mk = lambda: {k: v + 0.05 * torch.randn(v.shape, generator=gen) for k, v in init_mapper_state(64, 64, D).items()}
    sdo, sdv = mk(), mk()
    w_enc = fourier_frequencies([0.03, 2.0], 64, 0)
    w_enc_v = fourier_frequencies([0.03, 2.0] + [0.5] * 12, 64, 0)
    eng = InferenceEngine(cfg, uw, dw, cw, B, H, W, sdo, w_enc, 0.4, 0.2, mapper_view=sdv, w_enc_view=w_enc_v,
                          norm_scale_view=0.35, alpha_view=0.3)
    ph, phv = cfg.clip.vocab_size - 3, cfg.clip.vocab_size - 4
    ids = synth.input_ids(B, ph, cfg.clip.vocab_size, view_placeholder_id=phv)
    neg = synth.input_ids(1, ph, cfg.clip.vocab_size)
    neg[neg == ph] = 7  # a prompt without any placeholder
    eng.set_negative_prompt(neg)
    eng.set_prompt(ids, torch.full((B,), ph), torch.full((B,), phv), synth.gaussian((B, 12), 9).clamp(-1, 1))
    g = torch.Generator().manual_seed(31)
    _shared.update(eng=eng, lat=torch.randn(B, 4, H // 8, W // 8, generator=g),
                   noise=torch.randn(STEPS, B, 4, H // 8, W // 8, generator=g))
    return eng, _shared["lat"], _shared["noise"]


def _contexts_of(eng):
    nl = eng.cfg.unet.n_cross_layers
    d = {f"CONTEXT_TENSOR_{l}": eng.ctx_k[l].view(B, eng.L, -1).clone() for l in range(nl)}
    d.update({f"CONTEXT_TENSOR_BYPASS_{l}": eng.ctx_v[l].view(B, eng.L, -1).clone() for l in range(nl)})
    return d


@pytest.mark.parametrize("case", list(CASES))
def test_graph_eager_and_handed_in_contexts_agree_bit_for_bit(case, monkeypatch):
    from view_neti_amd import ops
    eng, lat, noise = _engine()
    kind, eta = CASES[case]
    kw = dict(eta=eta, step_noise=noise if eta else None, decode=False)
    x_graph = eng.generate(lat, STEPS, GS, kind, use_graph=True, **kw).cpu().clone()
    assert bool(torch.isfinite(x_graph).all()) and not torch.equal(x_graph, lat)
    # the eager run, with the conditioning of every step recorded as its sampler launch is issued
    recorded = []
    name = "cfg_sampler_step_noise" if eta else "cfg_sampler_step"
    real = getattr(ops, name)

    def recording(*a, **k):
        recorded.append(_contexts_of(eng))
        return real(*a, **k)

    monkeypatch.setattr(ops, name, recording)
    x_eager = eng.generate(lat, STEPS, GS, kind, use_graph=False, **kw).cpu().clone()
    monkeypatch.undo()
    assert len(recorded) == STEPS, "the eager loop launches the sampler kernel of its kind once per step"
    assert torch.equal(x_graph, x_eager), f"{case}: graph replay differs from the eager loop"
    x_ctx = eng.generate_from_contexts(lat, recorded, STEPS, GS, kind, **kw).cpu().clone()
    assert torch.equal(x_ctx, x_eager), f"{case}: generate_from_contexts on the recorded contexts differs from generate"
    assert not torch.equal(recorded[0]["CONTEXT_TENSOR_0"], recorded[1]["CONTEXT_TENSOR_0"])  # per-step conditioning


def test_captured_steps_are_cached_per_guidance_and_noise_term(monkeypatch):
    """two sampler kinds alternate on one engine: a call whose (guidance scale, noise term) was captured before replays
    that graph (the coefficients and timesteps live in device tables), another guidance scale captures anew"""
    eng, lat, noise = _engine()
    made = []
    real = torch.cuda.CUDAGraph

    def counting(*a, **k):
        made.append(1)
        return real(*a, **k)

    monkeypatch.setattr(torch.cuda, "CUDAGraph", counting)
    run = lambda kind, gs, eta=0.0: eng.generate(lat, STEPS, gs, kind, decode=False, eta=eta,
                                                 step_noise=noise if eta else None).cpu().clone()
    gs = 4.0  # no other test of this file uses it: the first two calls capture whatever ran before
    x_dpm = run("dpm++2m", gs)
    assert len(made) == 1
    x_eta = run("ddim", gs, 0.5)
    assert len(made) == 2
    assert torch.equal(run("dpm++2m", gs), x_dpm) and len(made) == 2
    x_ddim = run("ddim", gs)  # eta = 0: the same captured step as DPM-Solver++, other table rows
    assert len(made) == 2 and not torch.equal(x_ddim, x_dpm) and not torch.equal(x_ddim, x_eta)
    assert torch.equal(run("ddim", gs, 0.5), x_eta) and len(made) == 2
    x_g6 = run("dpm++2m", 6.0)
    assert len(made) == 3 and not torch.equal(x_g6, x_dpm)
    x_eta6 = run("ddim", 6.0, 0.5)
    assert len(made) == 4 and not torch.equal(x_eta6, x_eta)
