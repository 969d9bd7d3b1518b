"""Stochastic DDIM (eta > 0) on the GPU: the HIP step kernels vneti_cfg_sampler_step_noise / _noise_table against the
float64 restatement of DDIMScheduler.step (tests/helpers/ddim_eta_ref.py), their bit-identity with the eta = 0 kernel at
cn = 0, and `sd_pipeline_call(..., eta=...)` end to end on the tiny synthetic SD configs.

The file is precision-generic like tests/test_kernels_gpu.py: the 16-bit format is `lib.act_dtype()`.  A process computes in
ONE format, so the bf16 run of every case is a child pytest process with VNETI_PRECISION=bf16, started by the last test of
this file and checked through its junit report (no failure, no error, no skip, every collected case run).

Tolerance of the parity checks.  No number is stated here: each case first measures, on this GPU and these inputs, the error
of the EXISTING vneti_cfg_sampler_step against the same float64 restatement at eta = 0, and allows the new kernels 4x that
(the margin for the one extra fused multiply-add of cn * noise; the f32-rounded coefficients and the f32 arithmetic up to
that term are common to both).  Both the relative Frobenius error and the largest element error are held to it.
Every case prints its figures before it asserts (the "[ddim eta ...]" lines: the existing kernel's error, the new kernels'
error and their ratio).  NOT YET RECORDED: this file had no GPU run when it was written, so neither this comment nor
profiles/LAB_NOTES.md ("Stochastic DDIM") holds a measured value; a float32 host emulation of the same arithmetic put the
new kernels at 1.1 - 1.3x the existing kernel's relative error (4e-8 .. 6e-8) and at most 2.4x its largest element error.
"""
import os

import pytest
import torch

from helpers import ddim_eta_ref as R
from helpers.bf16_child import run_bf16_child
from helpers.checks import DEV, DT, TOL16, gen as _gen  # TOL16: unit roundoff of DT over fp16's (the factor behind t16)

pytestmark = pytest.mark.gpu

MARGIN = 4.0
STEPS = 5  # the 5-step DDIM schedule on the SD scaled_linear betas: timesteps 801, 601, 401, 201, 1


def _errs(got, ref64):
    d = got.double().cpu() - ref64
    return (d.norm() / ref64.norm()).item(), d.abs().max().item()


def _unpack(pred, B, Lc, HW):
    """NHWC [2 B HW][ld] 16-bit UNet output -> (uncond, cond), each [B][Lc][HW] float64 of the stored values"""
    p = pred[:, :Lc].double().cpu().view(2, B, HW, Lc).permute(0, 1, 3, 2)
    return p[0], p[1]


def _case(B, Lc, HW, seed):
    g = torch.Generator().manual_seed(seed)
    pred = torch.randn(2 * B * HW, 8, generator=g).to(DT)  # ld 8 > Lc: a view into a wider buffer, as the UNet's is
    x, m = torch.randn(B, Lc, HW, generator=g), torch.randn(B, Lc, HW, generator=g)
    noise = torch.randn(STEPS, B, Lc, HW, generator=g)
    return pred, x, m, noise


def _run(ops, form, pred_d, x, m, noise_d, coef, i, B, Lc, HW, gs, vpred):
    """one launch of the existing kernel (form 'base') or of a new entry; returns (x, m_prev, x_in) on the device"""
    xd, md = x.to(DEV).clone(), m.to(DEV).clone()
    x_in = torch.full((2 * B, Lc, HW), float("nan"), device=DEV)
    a_t, s_t, cx, c0, c1, cn = coef[i]
    p = pred_d[:, :Lc]
    if form == "base":
        ops.cfg_sampler_step(p, xd, md, x_in, B, Lc, HW, gs, a_t, s_t, cx, c0, c1, vpred)
    elif form == "scalar":
        ops.cfg_sampler_step_noise(p, xd, md, x_in, noise_d[i], B, Lc, HW, gs, a_t, s_t, cx, c0, c1, cn, vpred)
    else:
        table = torch.tensor(coef, dtype=torch.float32, device=DEV)
        step = torch.tensor([i], dtype=torch.int32, device=DEV)
        ops.cfg_sampler_step_noise_table(p, xd, md, x_in, B, Lc, HW, gs, table, noise_d, step, vpred)
    torch.cuda.synchronize()
    return xd, md, x_in


def _coef(eta):
    from view_neti_amd.engine.infer import ddim_eta_coefficients, inference_timesteps
    ac = R.scaled_linear_alphas_cumprod()
    ts = inference_timesteps("ddim", STEPS)
    return ac, ts, [ddim_eta_coefficients(ac, ts, i, eta) for i in range(STEPS)]


@pytest.mark.timeout(240)
@pytest.mark.parametrize("vpred", [False, True])
@pytest.mark.parametrize("gs", [1.0, 7.5])
@pytest.mark.parametrize("HW", [48 * 64, 72 * 96])
@pytest.mark.parametrize("B", [1, 4])
def test_noise_step_kernels_match_fp64(B, HW, gs, vpred):
    from view_neti_amd import ops
    Lc = 4
    pred, x, m, noise = _case(B, Lc, HW, 100 * B + HW % 97 + int(vpred))
    pred_d, noise_d = pred.to(DEV), noise.to(DEV)
    u, c = _unpack(pred, B, Lc, HW)
    e = R.guided(u, c, gs)
    ac, ts, coef0 = _coef(0.0)
    for i in (0, 2, 4):  # first, middle and last step (prev_t < 0: a_prev = alphas_cumprod[0])
        t, tp = ts[i], ts[i] - 1000 // STEPS
        # the yardstick: the existing kernel at eta = 0 against fp64, same inputs, this GPU
        ref_x, ref_x0 = R.ddim_step(ac, t, tp, x, e, 0.0, None, vpred)
        bx, bm, _ = _run(ops, "base", pred_d, x, m, noise_d, coef0, i, B, Lc, HW, gs, vpred)
        base_x, base_m = _errs(bx, ref_x), _errs(bm, ref_x0)
        print(f"[ddim eta B{B} HW{HW} g{gs} vpred{int(vpred)} step{i}] existing kernel, eta 0: x rel {base_x[0]:.3e} "
              f"max {base_x[1]:.3e}; x0 rel {base_m[0]:.3e} max {base_m[1]:.3e}")
        assert 0 < base_x[0] < 1e-5 and 0 < base_m[0] < 1e-5, "the yardstick itself is off"
        for eta in (0.3, 1.0):
            coef = _coef(eta)[2]
            ref_x, ref_x0 = R.ddim_step(ac, t, tp, x, e, eta, noise[i], vpred)
            for form in ("scalar", "table"):
                gx, gm, gin = _run(ops, form, pred_d, x, m, noise_d, coef, i, B, Lc, HW, gs, vpred)
                ex, em = _errs(gx, ref_x), _errs(gm, ref_x0)
                print(f"    eta {eta} {form:6s}: x rel {ex[0]:.3e} ({ex[0] / base_x[0]:.2f}x) max {ex[1]:.3e} "
                      f"({ex[1] / base_x[1]:.2f}x); x0 rel {em[0]:.3e} max {em[1]:.3e}")
                assert ex[0] <= MARGIN * base_x[0] and ex[1] <= MARGIN * base_x[1], (form, eta, i, ex, base_x)
                assert em[0] <= MARGIN * base_m[0] and em[1] <= MARGIN * base_m[1], (form, eta, i, em, base_m)
                for half in (gin[:B], gin[B:]):  # both CFG halves of the next UNet input
                    eh = _errs(half, ref_x)
                    assert eh[0] <= MARGIN * base_x[0] and eh[1] <= MARGIN * base_x[1] and torch.equal(half, gx)


@pytest.mark.timeout(120)
@pytest.mark.parametrize("vpred", [False, True])
@pytest.mark.parametrize("B,HW", [(1, 48 * 64), (4, 72 * 96), (2, 1001), (3, 7)])
def test_cn_zero_is_the_existing_kernel_bit_for_bit(B, HW, vpred):
    """cn = 0 (the eta = 0 row): x, m_prev and x_in of both new entries equal the existing kernel's byte for byte, on the
    16-byte path (HW a multiple of 4) and on the element path (HW = 1001, 7), whatever the noise buffer holds"""
    from view_neti_amd import ops
    Lc = 4
    pred, x, m, noise = _case(B, Lc, HW, 7 + HW)
    pred_d, noise_d = pred.to(DEV), noise.to(DEV)
    coef0 = _coef(0.0)[2]
    assert all(row[5] == 0.0 for row in coef0)
    for gs in (1.0, 7.5):
        for i in (0, 3, 4):
            want = _run(ops, "base", pred_d, x, m, noise_d, coef0, i, B, Lc, HW, gs, vpred)
            assert bool(torch.isfinite(want[2]).all())
            for form in ("scalar", "table"):
                got = _run(ops, form, pred_d, x, m, noise_d, coef0, i, B, Lc, HW, gs, vpred)
                for name, a, b in zip(("x", "m_prev", "x_in"), got, want):
                    assert torch.equal(a.view(torch.int32), b.view(torch.int32)), \
                        f"{form} B{B} HW{HW} g{gs} step{i}: {name} differs from vneti_cfg_sampler_step at cn = 0"


@pytest.mark.timeout(120)
@pytest.mark.parametrize("vpred", [False, True])
@pytest.mark.parametrize("B,HW", [(2, 48 * 64), (2, 1001)])
def test_cn_zero_is_bit_identical_with_a_history_term(B, HW, vpred):
    """DDIM rows have c1 = 0, which hides how c1 m_prev is folded in (one fma in the existing kernel).  Rows with
    c1 != 0, as a multistep sampler's, at cn = 0: still the existing kernel byte for byte, on both paths"""
    from view_neti_amd import ops
    Lc = 4
    pred, x, m, noise = _case(B, Lc, HW, 11 + HW)
    pred_d, noise_d = pred.to(DEV), noise.to(DEV)
    rows = [(0.8366, 0.5478, 0.6547, 1.3093, -0.4364, 0.0), (0.2512, 0.9679, 1.7, -0.83, 0.291, 0.0)]
    for gs in (1.0, 7.5):
        for i in range(len(rows)):
            want = _run(ops, "base", pred_d, x, m, noise_d, rows, i, B, Lc, HW, gs, vpred)
            for form in ("scalar", "table"):
                got = _run(ops, form, pred_d, x, m, noise_d, rows, i, B, Lc, HW, gs, vpred)
                for name, a, b in zip(("x", "m_prev", "x_in"), got, want):
                    assert torch.equal(a.view(torch.int32), b.view(torch.int32)), \
                        f"{form} HW{HW} g{gs} row{i}: {name} differs from vneti_cfg_sampler_step at cn = 0, c1 != 0"


@pytest.mark.timeout(120)
@pytest.mark.parametrize("vpred", [False, True])
def test_element_path_matches_fp64_and_the_table_row_is_the_step(vpred):
    """HW = 1001 (no multiple of 4: one element per thread) against fp64 under the same yardstick, and the table form reads
    row step[0] of BOTH tables: every step index gives the scalar entry's result for that step bit for bit"""
    from view_neti_amd import ops
    B, Lc, HW, gs, eta = 2, 4, 1001, 7.5, 1.0
    pred, x, m, noise = _case(B, Lc, HW, 31)
    pred_d, noise_d = pred.to(DEV), noise.to(DEV)
    u, c = _unpack(pred, B, Lc, HW)
    e = R.guided(u, c, gs)
    ac, ts, coef0 = _coef(0.0)
    coef = _coef(eta)[2]
    seen = []
    for i in range(STEPS):
        t, tp = ts[i], ts[i] - 1000 // STEPS
        bx, _, _ = _run(ops, "base", pred_d, x, m, noise_d, coef0, i, B, Lc, HW, gs, vpred)
        base = _errs(bx, R.ddim_step(ac, t, tp, x, e, 0.0, None, vpred)[0])
        ref_x, _ = R.ddim_step(ac, t, tp, x, e, eta, noise[i], vpred)
        sx, sm, sin_ = _run(ops, "scalar", pred_d, x, m, noise_d, coef, i, B, Lc, HW, gs, vpred)
        tx, tm, tin = _run(ops, "table", pred_d, x, m, noise_d, coef, i, B, Lc, HW, gs, vpred)
        ex = _errs(sx, ref_x)
        print(f"[ddim eta element path step{i} vpred{int(vpred)}] x rel {ex[0]:.3e} (existing, eta 0: {base[0]:.3e}) "
              f"max {ex[1]:.3e} ({base[1]:.3e})")
        assert ex[0] <= MARGIN * base[0] and ex[1] <= MARGIN * base[1]
        assert torch.equal(sx, tx) and torch.equal(sm, tm) and torch.equal(sin_, tin)
        seen.append(sx.cpu())
    assert all(not torch.equal(seen[i], seen[j]) for i in range(STEPS) for j in range(i))
    # the same rows through the 16-byte path
    HW = 48 * 64
    pred, x, m, noise = _case(B, Lc, HW, 32)
    pred_d, noise_d = pred.to(DEV), noise.to(DEV)
    for i in range(STEPS):
        s = _run(ops, "scalar", pred_d, x, m, noise_d, coef, i, B, Lc, HW, gs, vpred)
        t_ = _run(ops, "table", pred_d, x, m, noise_d, coef, i, B, Lc, HW, gs, vpred)
        assert all(torch.equal(a, b) for a, b in zip(s, t_))


@pytest.mark.timeout(60)
def test_launchers_refuse_bad_arguments():
    """the siblings' validation: null pointers, non-positive sizes, and the 2 GiB buffer-store bound (refused before any
    launch: the small buffers below are never touched)"""
    from view_neti_amd import ops
    B, Lc, HW = 1, 4, 64
    pred = torch.zeros(2 * B * HW, 8, dtype=DT, device=DEV)
    x, m = torch.zeros(B, Lc, HW, device=DEV), torch.zeros(B, Lc, HW, device=DEV)
    x_in, nz = torch.zeros(2 * B, Lc, HW, device=DEV), torch.zeros(2, B, Lc, HW, device=DEV)
    table, step = torch.zeros(2, 6, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    sc = (1.0, 0.8, 0.6, 0.9, 0.1, 0.0, 0.2, False)
    ops.cfg_sampler_step_noise(pred[:, :Lc], x, m, x_in, nz[0], B, Lc, HW, *sc)  # the well-formed call passes
    table[:, 0] = 0.8
    ops.cfg_sampler_step_noise_table(pred[:, :Lc], x, m, x_in, B, Lc, HW, 1.0, table, nz, step, False)
    torch.cuda.synchronize()
    bad_scalar = [dict(noise=None), dict(x=None), dict(m=None), dict(x_in=None), dict(B=0), dict(Lc=0), dict(HW=-4)]
    for kw in bad_scalar:
        a = dict(x=x, m=m, x_in=x_in, noise=nz[0], B=B, Lc=Lc, HW=HW)
        a.update(kw)
        with pytest.raises(RuntimeError, match="bad arguments"):
            ops.cfg_sampler_step_noise(pred[:, :Lc], a["x"], a["m"], a["x_in"], a["noise"], a["B"], a["Lc"], a["HW"], *sc)
    with pytest.raises(RuntimeError, match="bad arguments"):  # alpha_t = 0 divides
        ops.cfg_sampler_step_noise(pred[:, :Lc], x, m, x_in, nz[0], B, Lc, HW, 1.0, 0.0, 0.6, 0.9, 0.1, 0.0, 0.2, False)
    for kw in (dict(noise=None), dict(table=None), dict(step=None), dict(x_in=None), dict(B=-1), dict(HW=0)):
        a = dict(x_in=x_in, table=table, noise=nz, step=step, B=B, HW=HW)
        a.update(kw)
        with pytest.raises(RuntimeError, match="bad arguments"):
            ops.cfg_sampler_step_noise_table(pred[:, :Lc], x, m, a["x_in"], a["B"], Lc, a["HW"], 1.0, a["table"],
                                             a["noise"], a["step"], False)
    # B Lc HW 4 bytes = 2 GiB: one noise row (and x_in, twice that) is out of the buffer stores' range
    with pytest.raises(RuntimeError, match="2 GiB"):
        ops.cfg_sampler_step_noise_table(pred[:, :Lc], x, m, x_in, 1 << 14, 4, 1 << 13, 1.0, table, nz, step, False)
    with pytest.raises(RuntimeError, match="2 GiB"):  # x_in alone: B Lc HW 4 bytes = 1 GiB
        ops.cfg_sampler_step_noise(pred[:, :Lc], x, m, x_in, nz[0], 1 << 13, 4, 1 << 13, *sc)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------ end to end
_engines = {}


def _pipeline(cfg_name, B):
    """InferencePipeline on a tiny synthetic SD config (object + view mapper), one per (config, batch) and process"""
    if (cfg_name, B) in _engines:
        return _engines[(cfg_name, B)]
    from view_neti_amd import sd_config as sc, synth
    from view_neti_amd.compat.prompt_manager import PromptEmbeds
    from view_neti_amd.compat.sd_pipeline_call import InferencePipeline
    from view_neti_amd.compat.tokenizer import HashTokenizer
    from view_neti_amd.engine.infer import InferenceEngine
    from view_neti_amd.mapper import fourier_frequencies, init_mapper_state
    cfg = sc.CONFIGS[cfg_name]()
    D = cfg.clip.hidden_size
    uw, dw, cw = synth.unet_weights(cfg.unet), synth.vae_decoder_weights(cfg.vae), synth.clip_weights(cfg.clip)
    with torch.random.fork_rng(devices=[]):  # init_mapper_state draws from the global RNG: same mappers for every B
        torch.manual_seed(9)
        gen = torch.Generator().manual_seed(9)
        mk = lambda: {k: v + 0.05 * torch.randn(v.shape, generator=gen) for k, v in init_mapper_state(64, 64, D).items()}
        sdo, sdv = mk(), mk()
    w_enc = fourier_frequencies([0.03, 2.0], 64, 0)
    w_enc_v = fourier_frequencies([0.03, 2.0] + [0.5] * 12, 64, 0)
    eng = InferenceEngine(cfg, uw, dw, cw, B, 64, 64, sdo, w_enc, 0.4, 0.2, mapper_view=sdv, w_enc_view=w_enc_v,
                          norm_scale_view=0.35, alpha_view=0.3)
    ph, phv = cfg.clip.vocab_size - 3, cfg.clip.vocab_size - 4
    ids = synth.input_ids(1, ph, cfg.clip.vocab_size, view_placeholder_id=phv)
    emb = PromptEmbeds("synthetic", ids, torch.tensor([ph]), torch.tensor([phv]), synth.gaussian((1, 12), 9).clamp(-1, 1),
                       None, B)
    pipe = InferencePipeline(eng, HashTokenizer(cfg.clip.vocab_size), sampler="ddim")
    _engines[(cfg_name, B)] = (cfg, pipe, emb)
    return _engines[(cfg_name, B)]


# (not helpers.checks.frob_rel: this one compares in float64)
def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-20)).item()


@pytest.mark.timeout(300)
@pytest.mark.parametrize("cfg_name", ["tiny", "tiny21"])  # epsilon / v-prediction
def test_sd_pipeline_call_with_eta(cfg_name):
    from view_neti_amd.compat.sd_pipeline_call import sd_pipeline_call
    cfg, pipe, emb = _pipeline(cfg_name, 2)
    B, steps, gs = 2, 3, 5.0
    call = lambda eta, gen, **kw: sd_pipeline_call(pipe, emb, num_inference_steps=steps, guidance_scale=gs,
                                                   num_images_per_prompt=B, eta=eta, generator=gen, output_type="np",
                                                   return_dict=False, **kw)[0]
    img1 = call(1.0, _gen(3))
    x1 = pipe.engine.x.cpu().clone()
    assert img1.shape == (B, 64, 64, 3) and bool(torch.isfinite(torch.from_numpy(img1)).all()) and bool(torch.isfinite(x1).all())
    assert 0.0 <= img1.min() and img1.max() <= 1.0
    img0 = call(0.0, _gen(3))  # same initial latents (the first draw), no variance noise
    x0 = pipe.engine.x.cpu().clone()
    d_img, d_x = float(abs(img1 - img0).mean()), _rel(x1, x0)
    print(f"[sd_pipeline_call eta {cfg_name}] eta 1 vs eta 0: image mean abs diff {d_img:.3e}, final latents rel diff {d_x:.3e}")
    assert d_x > 0.1 and d_img > 0, "eta = 1 must change the sample"
    img1b = call(1.0, _gen(3))  # the captured noise-table step replays; equal generators: bit-identical
    assert (img1b == img1).all() and torch.equal(pipe.engine.x.cpu(), x1)
    img_half = call(0.5, _gen(3))  # another eta through the same graph: the table holds eta, not the capture
    assert not (img_half == img1).all() and not (img_half == img0).all()
    assert (call(1.0, _gen(3)) == img1).all()
    assert not (call(1.0, _gen(4)) == img1).all()
    # the reference's per-step prompt_embeds contract runs the eager noise step: same draws, finite, stochastic
    D = cfg.clip.hidden_size
    ctx = torch.randn(B, pipe.engine.L, D, generator=_gen(5)) * 0.3
    lat_a = sd_pipeline_call(pipe, ctx, num_inference_steps=steps, guidance_scale=gs, num_images_per_prompt=B, eta=1.0,
                             generator=_gen(3), output_type="latent").images.cpu()
    lat_b = sd_pipeline_call(pipe, ctx, num_inference_steps=steps, guidance_scale=gs, num_images_per_prompt=B, eta=1.0,
                             generator=_gen(3), output_type="latent").images.cpu()
    lat_0 = sd_pipeline_call(pipe, ctx, num_inference_steps=steps, guidance_scale=gs, num_images_per_prompt=B, eta=0.0,
                             generator=_gen(3), output_type="latent").images.cpu()
    assert bool(torch.isfinite(lat_a).all()) and torch.equal(lat_a, lat_b) and _rel(lat_a, lat_0) > 0.1


@pytest.mark.timeout(300)
@pytest.mark.parametrize("cfg_name", ["tiny", "tiny21"])
def test_batched_generators_match_single_sample_calls(cfg_name):
    """a list of B = 2 generators: sample i is the image of the B = 1 call with generator i (its own initial latents AND its
    own variance noise).  The bar is the one tests/test_nvs_gpu.py::test_batched_prompts_match_single_prompt_generations
    states for batched vs B = 1 generations (image mean abs err < 1e-2, final latents rel < 2e-2, fp16), times the ratio
    of the unit roundoffs in bf16 as everywhere in the kernel files."""
    from view_neti_amd.compat.sd_pipeline_call import sd_pipeline_call
    _, pipe2, emb2 = _pipeline(cfg_name, 2)
    _, pipe1, emb1 = _pipeline(cfg_name, 1)
    steps, gs, seeds = 3, 5.0, [3, 5]
    img = sd_pipeline_call(pipe2, emb2, num_inference_steps=steps, guidance_scale=gs, num_images_per_prompt=2, eta=1.0,
                           generator=[_gen(s) for s in seeds], output_type="np", return_dict=False)[0]
    x = pipe2.engine.x.cpu().clone()
    worst_img, worst_x = 0.0, 0.0
    for b, s in enumerate(seeds):
        ib = sd_pipeline_call(pipe1, emb1, num_inference_steps=steps, guidance_scale=gs, num_images_per_prompt=1, eta=1.0,
                              generator=_gen(s), output_type="np", return_dict=False)[0]
        worst_img = max(worst_img, float(abs(img[b] - ib[0]).mean()))
        worst_x = max(worst_x, _rel(x[b], pipe1.engine.x[0]))
    cross = _rel(x[0], x[1])
    print(f"[batched generators {cfg_name}] vs B=1: image mean abs err max {worst_img:.3e}; final latents rel max "
          f"{worst_x:.3e} (sample 0 vs sample 1: {cross:.3e})")
    assert worst_img < 1e-2 * TOL16 and worst_x < 2e-2 * TOL16
    assert cross > 0.5, "two generators, two samples"
    with pytest.raises(ValueError):
        sd_pipeline_call(pipe2, emb2, num_inference_steps=steps, guidance_scale=gs, num_images_per_prompt=2, eta=1.0,
                         generator=[_gen(1)], output_type="np")


@pytest.mark.timeout(300)
@pytest.mark.parametrize("cfg_name", ["tiny", "tiny21"])
def test_latents_after_three_steps_match_a_host_loop(cfg_name, monkeypatch):
    """the engine's eager loop at eta = 1 with its UNet outputs recorded at each step; a float64 host loop (the restatement,
    the same generator draws, the recorded outputs) must land on the engine's final latents.  Yardstick as in the kernel
    parity test, for the same three chained steps: the EXISTING kernel at eta = 0 on the same recorded outputs against
    the float64 loop at eta = 0; the eta = 1 loop may be 4x that far off.  The captured (noise-table) loop equals the eager
    one bit for bit."""
    from view_neti_amd import ops
    from view_neti_amd.compat.sd_pipeline_call import get_neg_prompt_input_ids
    from view_neti_amd.engine.infer import ddim_eta_coefficients, inference_timesteps
    cfg, pipe, emb = _pipeline(cfg_name, 2)
    eng = pipe.engine
    B, Lc, h, w, steps, gs, eta = 2, eng.Lc, eng.h, eng.w, 3, 5.0, 1.0
    HW = h * w
    vpred = cfg.ddpm.prediction_type == "v_prediction"
    g = _gen(21)
    lat = torch.randn(B, Lc, h, w, generator=g)
    noise = torch.stack([torch.randn(B, Lc, h, w, generator=g) for _ in range(steps)])
    eng.set_negative_prompt(get_neg_prompt_input_ids(pipe).input_ids)
    rep = lambda t: t.expand(B, *t.shape[1:]) if t.dim() > 1 else t.expand(B)
    eng.set_prompt(rep(emb.input_ids), rep(emb.input_ids_placeholder_object), rep(emb.input_ids_placeholder_view),
                   rep(emb.view_params))
    preds, real = [], ops.cfg_sampler_step_noise

    def recording(pred, *a):
        preds.append(pred.clone())
        return real(pred, *a)

    monkeypatch.setattr(ops, "cfg_sampler_step_noise", recording)
    eng.generate(lat.to(DEV), steps, gs, "ddim", decode=False, use_graph=False, eta=eta, step_noise=noise)
    monkeypatch.undo()
    x_eager = eng.x.cpu().clone()
    assert len(preds) == steps and bool(torch.isfinite(x_eager).all())
    eng.generate(lat.to(DEV), steps, gs, "ddim", decode=False, eta=eta, step_noise=noise)
    assert torch.equal(eng.x.cpu(), x_eager), "graph replay of the noise-table step must match the eager loop bit for bit"
    ac = eng.ac.double().cpu()
    ts = inference_timesteps("ddim", steps, cfg.ddpm.num_train_timesteps)
    ratio = cfg.ddpm.num_train_timesteps // steps
    # float64 loops on the recorded outputs: eta = 1 (the claim) and eta = 0 (the yardstick's reference)
    x1 = lat.double().view(B, Lc, HW)
    xb = x1.clone()
    bx, bm = lat.view(B, Lc, HW).to(DEV).clone(), torch.zeros(B, Lc, HW, device=DEV)
    b_in = torch.zeros(2 * B, Lc, HW, device=DEV)
    for i, t in enumerate(ts):
        u, c = _unpack(preds[i], B, Lc, HW)
        e = R.guided(u, c, gs)
        x1, _ = R.ddim_step(ac, t, t - ratio, x1, e, eta, noise[i].view(B, Lc, HW), vpred)
        xb, _ = R.ddim_step(ac, t, t - ratio, xb, e, 0.0, None, vpred)
        a_t, s_t, cx, c0, c1, _ = ddim_eta_coefficients(ac, ts, i, 0.0)
        ops.cfg_sampler_step(preds[i], bx, bm, b_in, B, Lc, HW, gs, a_t, s_t, cx, c0, c1, vpred)
    torch.cuda.synchronize()
    base = _errs(bx, xb)
    got = _errs(x_eager.view(B, Lc, HW), x1)
    print(f"[ddim eta host loop {cfg_name}] final latents vs fp64 after {steps} steps: rel {got[0]:.3e} max {got[1]:.3e}; "
          f"existing kernel, eta 0, same outputs: rel {base[0]:.3e} max {base[1]:.3e}")
    assert 0 < base[0] < 1e-4
    assert got[0] <= MARGIN * base[0] and got[1] <= MARGIN * base[1]


@pytest.mark.timeout(120)
def test_eta_with_dpm_solver_raises():
    from view_neti_amd.compat.sd_pipeline_call import InferencePipeline, sd_pipeline_call
    _, pipe, emb = _pipeline("tiny", 2)
    dpm = InferencePipeline(pipe.engine, pipe.tokenizer, sampler="dpm++2m")
    with pytest.raises(ValueError, match="ignores"):
        sd_pipeline_call(dpm, emb, num_inference_steps=3, guidance_scale=5.0, num_images_per_prompt=2, eta=0.5,
                         generator=_gen(0))
    with pytest.raises(ValueError):
        pipe.engine.generate(torch.zeros(2, 4, 8, 8, device=DEV), 3, 5.0, "dpm++2m", eta=0.5)
    with pytest.raises(ValueError):
        pipe.engine.generate(torch.zeros(2, 4, 8, 8, device=DEV), 3, 5.0, "ddim", eta=1.0,
                             step_noise=torch.zeros(2, 2, 4, 8, 8))  # T = 3 rows wanted
    eng = pipe.engine
    eng.generate(torch.zeros(2, 4, 8, 8, device=DEV), 3, 5.0, "ddim", eta=1.0, decode=False)  # noise: the global generator
    assert bool(torch.isfinite(eng.x).all()) and eng.noise_table.shape[0] >= 3
    assert eng.memory_bytes() == eng.unet.bytes + eng.text.bytes + eng.decoder.bytes + eng.noise_table.numel() * 4
    # eta = 0 with dpm++2m stays what it was
    out = sd_pipeline_call(dpm, emb, num_inference_steps=3, guidance_scale=5.0, num_images_per_prompt=2, eta=0.0,
                           generator=_gen(0), output_type="np", return_dict=False)[0]
    assert out.shape == (2, 64, 64, 3)


# ------------------------------------------------------------------------------------------ the bf16 library
@pytest.mark.timeout(300)
def test_every_case_against_the_bf16_library(tmp_path):
    """the cases above in a child process with VNETI_PRECISION=bf16 (libvneti_hip_bf16.so); one child, under its own time
    limit, nothing retried"""
    out = run_bf16_child(os.path.join("tests", os.path.basename(__file__)), "not bf16_library", 170, tmp_path, least=30,
                         extra_args=("-s",), collect_limit=120, what="ddim eta bf16")
    print("\n".join(l for l in out.splitlines() if l.startswith("[") or l.startswith("    eta")))
