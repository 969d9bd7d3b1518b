"""Min-SNR loss weighting and offset noise on the GPU: the two kernels through the C ABI, the
whole step against the CPU oracle, and the engine / Coach behaviour around them.

References.  Kernels: the float64 restatement of tests/helpers/loss_options_ref.py from the same 16-bit-rounded inputs and
the same f32 alphas_cumprod table, at the bars of test_elementwise_mse_loss_grad / test_elementwise_sample_add_noise
(tests/test_kernels_gpu.py): loss_sum 1e-5 relative, dpred t16(1e-3), the f32 outputs 1e-5.  Whole step: the unchanged
oracle (oracle/sd_ref.py::train_step_loss) fed the offset noise, with the weighted loss formed from its prediction, at the
bars of test_train_step_tiny_matches_oracle.  Everything the options must NOT change is compared for bit equality.  The
kernel cases (test_kernel_*) also run against libvneti_hip_bf16.so in a child process."""
import json
import math
import os

import pytest
import torch

from helpers import coach_runs as rt  # the tiny Coach runs: toys, mode0_cfg, coach, train_counting
from helpers import loss_options_ref as LR
from helpers.bf16_child import run_bf16_child
from helpers.checks import DEV, DT, check, rnd, t16, ops as _ops
from helpers.engines import FORMS, STATE, build_device_rng_engine as _build, build_train_engine as build_step
from helpers.engines import feed_device_rng, feed_six as _feed, run_steps, six_steps as _six_steps, snapshot

pytestmark = pytest.mark.gpu
F32 = torch.float32
GAMMA, OFFSET = 5.0, 0.1
AC = LR.scaled_linear_alphas_cumprod_f32()   # the f32 table: the shared input of kernel and reference
B, H, W = 2, 64, 64   # of the device-RNG engines (helpers.engines.build_device_rng_engine)
ROWS = 16


# ================================================================================================ kernel: mse_loss_grad_snr
def _mse_inputs(Bn, Lc, HW, ld):
    pbig = rnd(Bn * HW, ld, seed=84)
    target = rnd(Bn, Lc, HW, seed=85, dtype=F32)
    return pbig, target


def _mse_launch(entry, pbig, target, Bn, Lc, HW, scale, start, *extra):
    """one launch on strided 4-of-ld-column views; -> (dbig with 7.0 beyond the channels, loss_sum)"""
    ops = _ops()
    dbig = torch.full(tuple(pbig.shape), 7.0, dtype=DT, device=DEV)
    loss_sum = torch.tensor([start], dtype=F32, device=DEV)
    getattr(ops, entry)(pbig.to(DEV)[:, :Lc], target.to(DEV), dbig[:, :Lc], loss_sum, torch.tensor([scale], device=DEV),
                        Bn, Lc, HW, *extra)
    torch.cuda.synchronize()
    return dbig, loss_sum


@pytest.mark.parametrize("vpred", [False, True], ids=["epsilon", "v-prediction"])
@pytest.mark.parametrize("Bn,HW,t", [(3, 81, (0, 146, 147)), (3, 81, (999, 500, 146)), (1, 1, (40,))],
                         ids=["t0-146-147", "t999-500-146", "one-pixel"])
def test_kernel_mse_loss_grad_snr_against_float64(Bn, HW, t, vpred):
    """N = 972 (a partly filled last block of four) and N = 4; pred / dpred are 4 of 8 strided columns, the loss scale is
    128, loss_sum starts at 3.25; timesteps on both sides of the gamma = 5 boundary (146 | 147) and at both ends"""
    Lc, ld, scale, start = 4, 8, 128.0, 3.25
    pbig, target = _mse_inputs(Bn, Lc, HW, ld)
    tt = torch.tensor(t, dtype=torch.int64)
    dbig, loss_sum = _mse_launch("mse_loss_grad_snr", pbig, target, Bn, Lc, HW, scale, start, tt.to(DEV), AC.to(DEV), GAMMA,
                                 vpred)
    w = LR.min_snr_weight(AC, tt, GAMMA, vpred)
    if not vpred:
        assert [float(x) == 1.0 for x in w] == [int(x) >= 147 for x in t]  # the cases sit where they are meant to
    pr = pbig[:, :Lc].double().view(Bn, HW, Lc).permute(0, 2, 1)   # NCHW
    d = pr - target.double()
    wsum = (w.view(-1, 1, 1) * d * d).sum()
    loss, grad = LR.weighted_mse(pr.unsqueeze(-1), target.unsqueeze(-1), w)
    name = f"mse_snr Bn{Bn} HW{HW} t{t} vpred{int(vpred)}"
    check(f"{name} loss_sum", loss_sum, (start + wsum).reshape(1), 1e-5)
    if Bn * Lc * HW == 972:  # (as test_elementwise_mse_loss_grad: at N = 4 the f32 rounding of 3.25 + sum is the whole error)
        check(f"{name} loss (mean)", (loss_sum.cpu().double() - start) / (Bn * Lc * HW), loss.reshape(1), 1e-5)
    check(f"{name} dpred", dbig[:, :Lc].view(Bn, HW, Lc), (grad.squeeze(-1) * scale).permute(0, 2, 1), t16(1e-3))
    assert bool((dbig[:, Lc:] == 7).all()), "columns beyond Lc were written"
    if not vpred and any(int(x) < 147 for x in t):  # the weighting is not a no-op in this case
        plain, _ = _mse_launch("mse_loss_grad", pbig, target, Bn, Lc, HW, scale, start)
        assert not torch.equal(plain, dbig)


@pytest.mark.parametrize("Bn,HW", [(3, 81), (1, 1)], ids=["four-blocks", "one-block"])
def test_kernel_mse_loss_grad_snr_gamma_inf_is_the_unweighted_kernel(Bn, HW):
    """epsilon, gamma = +inf: w = snr / snr = 1 exactly, multiplied in — dpred bit for bit; loss_sum bit for bit where one
    block adds to it, at the 1e-5 bar where four blocks add with float atomics in any order"""
    Lc, ld, scale, start = 4, 8, 128.0, 3.25
    pbig, target = _mse_inputs(Bn, Lc, HW, ld)
    t = torch.tensor([0, 999, 146][:Bn], dtype=torch.int64)
    d0, s0 = _mse_launch("mse_loss_grad", pbig, target, Bn, Lc, HW, scale, start)
    d1, s1 = _mse_launch("mse_loss_grad_snr", pbig, target, Bn, Lc, HW, scale, start, t.to(DEV), AC.to(DEV), math.inf, False)
    assert torch.equal(d0, d1), "gamma = inf changed dpred"
    if Bn * Lc * HW <= 256:
        assert torch.equal(s0, s1), (s0.item(), s1.item())
    else:
        check("mse_snr gamma=inf loss_sum", s1, s0.double(), 1e-5)


def test_kernel_mse_loss_grad_snr_refuses_bad_arguments():
    pbig, target = _mse_inputs(1, 4, 1, 8)
    t = torch.zeros(1, dtype=torch.int64, device=DEV)
    for gamma in (0.0, -1.0, math.nan):
        with pytest.raises(RuntimeError, match="gamma"):
            _mse_launch("mse_loss_grad_snr", pbig, target, 1, 4, 1, 1.0, 0.0, t, AC.to(DEV), gamma, False)


# ================================================================================================ kernel: sample_add_noise_offset
def _noise_inputs():
    """the inputs of test_elementwise_sample_add_noise, plus the (Bn, Lc) offset draw"""
    Bn, Lc, HW, ldm = 3, 4, 81, 16
    mbig = rnd(Bn * HW, ldm, seed=80)
    mbig[:, Lc:2 * Lc] = (rnd(Bn * HW, Lc, seed=81).float() * 2 - 3).to(DT)
    mbig[:6, Lc:2 * Lc] = torch.tensor([[-40.0, 25.0, -30.0, 20.0]] * 6, dtype=DT)
    eps = rnd(Bn, Lc, HW, seed=82, dtype=F32)
    noise = rnd(Bn, Lc, HW, seed=83, dtype=F32)
    offs = rnd(Bn, Lc, seed=87, dtype=F32)
    t = torch.tensor([0, 999, 500], dtype=torch.int64)
    return Bn, Lc, HW, mbig, eps, noise, offs, t


def _noise_launch(mbig, eps, noise, t, vpred, Bn, Lc, HW, offs=None, offset=None, scaling=0.18215):
    ops = _ops()
    outs = [torch.full((Bn, Lc, HW), float("nan"), dtype=F32, device=DEV) for _ in range(3)]
    nd = noise.to(DEV)
    a = (mbig.to(DEV)[:, :2 * Lc], eps.to(DEV), nd, t.to(DEV), AC.to(DEV), scaling, vpred, *outs, Bn, Lc, HW)
    if offs is None:
        ops.sample_add_noise(*a)
    else:
        ops.sample_add_noise_offset(*a, offs.to(DEV), offset)
    torch.cuda.synchronize()
    assert torch.equal(nd.cpu(), noise), "the noise input buffer was modified"
    return outs


@pytest.mark.parametrize("vpred", [False, True], ids=["epsilon", "v-prediction"])
def test_kernel_sample_add_noise_offset_zero_is_the_plain_kernel(vpred):
    Bn, Lc, HW, mbig, eps, noise, offs, t = _noise_inputs()
    plain = _noise_launch(mbig, eps, noise, t, vpred, Bn, Lc, HW)
    zero = _noise_launch(mbig, eps, noise, t, vpred, Bn, Lc, HW, offs * 1e6, 0.0)
    for a, b, what in zip(plain, zero, ("latents", "noisy", "target")):
        assert torch.equal(a, b), f"offset = 0 changed {what}"


@pytest.mark.parametrize("vpred", [False, True], ids=["epsilon", "v-prediction"])
def test_kernel_sample_add_noise_offset_against_float64(vpred):
    """offset 0.1 at t = (0, 999, 500), Bn 3, Lc 4, HW 81, moments a 8-of-16-column view; all outputs f32: the 1e-5 bar"""
    Bn, Lc, HW, mbig, eps, noise, offs, t = _noise_inputs()
    scaling = 0.18215
    lat, noisy, target = _noise_launch(mbig, eps, noise, t, vpred, Bn, Lc, HW, offs, OFFSET, scaling)
    mm = mbig[:, :2 * Lc].double().view(Bn, HW, 2 * Lc).permute(0, 2, 1)      # NCHW
    z = (mm[:, :Lc] + torch.exp(0.5 * mm[:, Lc:].clamp(-30, 20)) * eps.double()) * float(torch.tensor(scaling).float())
    n2 = LR.offset_noise(noise.unsqueeze(-1), offs, float(torch.tensor(OFFSET).float())).squeeze(-1)
    want_noisy, want_target = LR.add_noise(z.unsqueeze(-1), n2.unsqueeze(-1), AC, t, vpred)
    check(f"offset latents vpred{int(vpred)}", lat, z, 1e-5)
    check(f"offset noisy vpred{int(vpred)}", noisy, want_noisy.squeeze(-1), 1e-5)
    check(f"offset target vpred{int(vpred)}", target, want_target.squeeze(-1), 1e-5)
    plain = _noise_launch(mbig, eps, noise, t, vpred, Bn, Lc, HW)
    assert torch.equal(plain[0], lat) and not torch.equal(plain[1], noisy) and not torch.equal(plain[2], target)
    if not vpred:  # for epsilon the target IS the offset noise: one fma per element
        assert torch.equal(target.cpu(), torch.addcmul(noise.double(), torch.tensor(OFFSET).float().double(),
                                                       offs.double()[:, :, None]).float())


def test_bf16_library_runs_the_kernel_cases(tmp_path):
    """the test_kernel_* cases above against libvneti_hip_bf16.so, in a child pytest process with VNETI_PRECISION=bf16 (a
    process computes in one 16-bit format): no failure, no error, nothing skipped, as many cases as were collected"""
    from view_neti_amd import lib
    if lib.precision() == "bf16":
        return  # this IS the bf16 run
    run_bf16_child(os.path.join("tests", os.path.basename(__file__)), "test_kernel_", 240, tmp_path, least=13)


# ================================================================================================ whole step vs the CPU oracle
_ORACLE = {}


def _oracle(cfg_name, with_view, H, W, offset_on):
    """the oracle's forward on (noise + s xi) or on the plain noise, once per (family, offset) and left unchanged:
    -> dict(pred with its graph, target, parameter leaves, weights of the batch's timesteps)"""
    key = (cfg_name, offset_on)
    if key in _ORACLE:
        return _ORACLE[key]
    from oracle import sd_ref as R
    from view_neti_amd import synth
    B = 2
    cfg, _, (uw, vw, cw), sd, w_enc, extra = _STEP_BUILDS[cfg_name]
    ph, phv = cfg.clip.vocab_size - 3, cfg.clip.vocab_size - 4
    inp = _step_inputs(cfg, with_view, H, W)
    noise = inp["noise"] + OFFSET * inp["xi"][:, :, None, None] if offset_on else inp["noise"]
    r16 = lambda d: {k: (v.half().float() if v.dim() >= 2 and "embedding" not in k else v) for k, v in d.items()}
    p_o = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    leaves, view = [p_o], None
    if with_view:
        p_v = {k: v.clone().requires_grad_(True) for k, v in extra["mapper_view"].items()}
        leaves.append(p_v)
        view = dict(p=p_v, w_enc=extra["w_enc_view"], norm_scale=0.35, placeholder=torch.full((B,), phv),
                    params=inp["vparams"], alpha=0.3, unconstrained=False)
    _, aux = R.train_step_loss(cfg, r16(uw), r16(vw), r16(cw), p_o, w_enc, 0.4, inp["px"], inp["ids"], torch.full((B,), ph),
                               inp["t"], inp["eps"], noise, alpha=0.2, view=view)
    vpred = cfg.ddpm.prediction_type == "v_prediction"
    ac = R.alphas_cumprod(cfg.ddpm)
    target = R.get_velocity(ac, aux["latents"], noise, inp["t"]) if vpred else noise
    _ORACLE[key] = dict(pred=aux["pred"], target=target, leaves=leaves, vpred=vpred)
    return _ORACLE[key]


def _oracle_loss_and_grad(o, w):
    """mean_b(w_b mean_chw(d^2)) of the oracle's prediction and its mapper gradient (the graph is kept for the next call)"""
    from view_neti_amd.engine.text import flatten_mapper_state
    per_sample = ((o["pred"].float() - o["target"].float()) ** 2).mean(dim=(1, 2, 3))
    loss = (w.float() * per_sample).mean()
    flat = [v for p in o["leaves"] for v in p.values()]
    grads = torch.autograd.grad(loss, flat, retain_graph=True)
    out, i = [], 0
    for p in o["leaves"]:
        out.append(flatten_mapper_state({k: g for k, g in zip(p, grads[i:i + len(p)])}))
        i += len(p)
    return loss.item(), torch.cat(out)


_STEP_BUILDS = {}
T_STEP = (40, 700)  # gamma = 5 clips the first (snr ~ 32) and not the second (snr ~ 0.09)


def _step_inputs(cfg, with_view, H, W):
    from view_neti_amd import synth
    B = 2
    ph, phv = cfg.clip.vocab_size - 3, cfg.clip.vocab_size - 4
    return dict(ids=synth.input_ids(B, ph, cfg.clip.vocab_size, view_placeholder_id=phv if with_view else None),
                px=synth.pixel_values(B, H, W), t=torch.tensor(T_STEP, dtype=torch.int64),
                eps=synth.gaussian((B, 4, H // 8, W // 8), 3), noise=synth.gaussian((B, 4, H // 8, W // 8), 4),
                xi=synth.gaussian((B, 4), 6), vparams=synth.gaussian((B, 12), 9).clamp(-1, 1) if with_view else None)


def _bars(loss_gpu, g_gpu, loss_ref, g_ref):
    rel = abs(loss_gpu - loss_ref) / loss_ref
    cos = torch.nn.functional.cosine_similarity(g_gpu, g_ref, dim=0).item()
    gerr = ((g_gpu - g_ref).norm() / g_ref.norm()).item()
    return rel, cos, gerr


@pytest.mark.parametrize("snr_on,offset_on", [(True, True), (True, False), (False, True)], ids=["both", "snr", "offset"])
@pytest.mark.parametrize("cfg_name,with_view,H,W", [("tiny", False, 64, 64), ("tiny21", True, 64, 128)],
                         ids=["tiny-epsilon", "tiny21-v-view"])
def test_train_step_with_options_matches_oracle(cfg_name, with_view, H, W, snr_on, offset_on):
    """B = 2, t = (40, 700), gamma 5, offset 0.1: weighted loss within 1e-3 relative, mapper-gradient cosine > 0.999 and
    relative error < 5e-2 (the bars of test_train_step_tiny_matches_oracle) — and NOT within them of the plain objective"""
    B = 2
    kw = dict(snr_gamma=GAMMA if snr_on else None, noise_offset=OFFSET if offset_on else None)
    cfg, eng, weights, sd, w_enc, extra = build_step(cfg_name, B, H, W, with_view=with_view, device_rng=False, lr=4e-3, **kw)
    _STEP_BUILDS.setdefault(cfg_name, (cfg, None, weights, sd, w_enc, extra))
    inp = _step_inputs(cfg, with_view, H, W)
    ph, phv = cfg.clip.vocab_size - 3, cfg.clip.vocab_size - 4
    eng.set_batch(inp["px"], inp["ids"], torch.full((B,), ph), torch.full((B,), phv) if with_view else None, inp["vparams"])
    if offset_on:
        with pytest.raises(ValueError, match="offset_noise"):
            eng.set_noise(inp["eps"], inp["noise"], inp["t"])
        eng.set_noise(inp["eps"], inp["noise"], inp["t"], offset_noise=inp["xi"])
    else:
        with pytest.raises(ValueError, match="offset_noise"):
            eng.set_noise(inp["eps"], inp["noise"], inp["t"], offset_noise=inp["xi"])
        eng.set_noise(inp["eps"], inp["noise"], inp["t"])
    noise_before = eng.noise.clone()
    eng.forward_backward()
    torch.cuda.synchronize()
    assert torch.equal(eng.noise, noise_before)
    loss_gpu, g_gpu = eng.loss(), (eng.grads / eng.scaler[0]).float().cpu()
    o = _oracle(cfg_name, with_view, H, W, offset_on)
    ones = torch.ones(B, dtype=torch.float64)
    w = LR.min_snr_weight(AC, inp["t"], GAMMA, o["vpred"]) if snr_on else ones
    rel, cos, gerr = _bars(loss_gpu, g_gpu, *_oracle_loss_and_grad(o, w))
    plain = _bars(loss_gpu, g_gpu, *_oracle_loss_and_grad(_oracle(cfg_name, with_view, H, W, False), ones))
    print(f"[options step {cfg_name} snr={snr_on} offset={offset_on}] w {w.tolist()} loss gpu {loss_gpu:.6f} rel {rel:.2e}; "
          f"grad cos {cos:.6f} rel {gerr:.2e}; against the plain objective: loss rel {plain[0]:.2e} cos {plain[1]:.6f} "
          f"rel {plain[2]:.2e}")
    assert rel < 1e-3, "the weighted loss must match the oracle to 1e-3 relative"
    assert cos > 0.999 and gerr < 5e-2
    assert not (plain[0] < 1e-3 and plain[1] > 0.999 and plain[2] < 5e-2), "the step passes with the option ignored"


# ================================================================================================ engine behaviour
def test_snr_gamma_inf_is_the_plain_training():
    """epsilon family, captured steps: every weight is exactly 1, so every state tensor is the plain engine's"""
    plain, _, _ = _six_steps("one-mapper")
    inf, _, _ = _six_steps("one-mapper", snr_gamma=math.inf)
    for f in STATE:
        assert torch.equal(plain[f], inf[f]), f"{f} differs with snr_gamma=inf"
    five, _, _ = _six_steps("one-mapper", snr_gamma=GAMMA)
    assert not torch.equal(plain["params"], five["params"]), "snr_gamma=5 must change the training"
    for f in ("rng_state", "opt_step"):
        assert torch.equal(plain[f], five[f])


def test_device_rng_streams():
    """stream 5 draws the offset; streams 0-2 draw what they always drew"""
    ops = _ops()
    cfg, plain = _build(False, 1)
    _, eng = _build(False, 1, noise_offset=OFFSET)
    assert plain.offset_noise is None and tuple(eng.offset_noise.shape) == (B, 4)
    draws = []
    for s in range(2):
        state = eng.rng_state.clone()
        for e in (plain, eng):
            _feed(cfg, e, s, 0, False)
            assert e.step()
        torch.cuda.synchronize()
        if s == 0:
            for f in ("timesteps", "eps", "noise", "latents"):
                assert torch.equal(getattr(plain, f), getattr(eng, f)), f"{f} differs with noise_offset on"
            assert not torch.equal(plain.target, eng.target)
            # epsilon: the target is noise + s * offset_noise
            want = torch.addcmul(eng.noise.double(), torch.tensor(OFFSET).float().double().to(DEV),
                                 eng.offset_noise.double()[:, :, None, None]).float()
            assert torch.equal(eng.target, want)
        ops.rng_advance(state)
        direct = torch.zeros_like(eng.offset_noise)
        ops.rng_fill_normal(direct, state, 5)
        torch.cuda.synchronize()
        assert torch.equal(state, eng.rng_state) and torch.equal(direct, eng.offset_noise)
        for other in (1, 2):
            ops.rng_fill_normal(direct, state, other)
            assert not torch.equal(direct, eng.offset_noise)
        draws.append(eng.offset_noise.clone())
    assert not torch.equal(draws[0], draws[1]) and float(draws[0].abs().max()) > 0


_BOTH = dict(snr_gamma=GAMMA, noise_offset=OFFSET)


@pytest.mark.parametrize("form", ["one-mapper", "mode3"])
def test_captured_replay_equals_eager_and_resumes(form):
    """both options on: 3 eager steps == 3 replayed steps; state_dict after 3 -> a fresh engine -> 3 more == 6 in one run;
    a state is refused by an engine without the option or with another value, naming the field"""
    mode3 = FORMS[form][0]
    cfg, eager = _build(mode3, 1, **_BOTH)
    for s in range(3):
        _feed(cfg, eager, s, 0, mode3)
        assert eager.step_eager()
    _, graph = _build(mode3, 1, **_BOTH)
    _feed(cfg, graph, 0, 0, mode3)
    graph.capture()
    assert graph.graph_a is not None
    run_steps(cfg, graph, range(3), mode3, _feed)
    a, b = snapshot(eager, STATE), snapshot(graph, STATE)
    for f in STATE:
        assert torch.equal(a[f], b[f]), f"{form}: {f} differs between eager and replayed steps"
    assert eager.loss() == graph.loss()
    sd = graph.state_dict()
    assert sd["meta"]["snr_gamma"] == GAMMA and sd["meta"]["noise_offset"] == OFFSET
    run_steps(cfg, graph, range(3, 6), mode3, _feed)
    want = snapshot(graph, STATE)
    _, fresh = _build(mode3, 1, **_BOTH)
    fresh.load_state_dict(sd)
    _feed(cfg, fresh, 3, 0, mode3)
    fresh.capture()
    run_steps(cfg, fresh, range(3, 6), mode3, _feed)
    got = snapshot(fresh, STATE)
    for f in STATE:
        assert torch.equal(want[f], got[f]), f"{form}: {f} differs after the resume"
    if mode3:
        return
    for field, other in (("snr_gamma", dict(_BOTH, snr_gamma=None)), ("snr_gamma", dict(_BOTH, snr_gamma=4.0)),
                         ("noise_offset", dict(_BOTH, noise_offset=None)), ("noise_offset", dict(_BOTH, noise_offset=0.2))):
        _, e = _build(False, 1, **other)
        with pytest.raises(ValueError, match=field) as err:
            e.load_state_dict(sd)
        assert "n_params" not in str(err.value)
        with pytest.raises(ValueError, match=field):
            fresh.load_state_dict(e.state_dict())
    _, plain = _build(False, 1)
    assert "snr_gamma" not in plain.state_dict()["meta"] and "noise_offset" not in plain.state_dict()["meta"]


def test_constructor_refuses_bad_values():
    for name in ("snr_gamma", "noise_offset"):
        for bad in (0.0, -1.0, math.nan):
            with pytest.raises(ValueError, match=name):
                _build(False, 1, **{name: bad})
    with pytest.raises(ValueError, match="noise_offset"):
        _build(False, 1, noise_offset=math.inf)


def test_heldout_losses_and_the_ring_stay_unweighted():
    from view_neti_amd import synth
    ops = _ops()
    cfg, plain = _build(False, 1)
    _, eng = _build(False, 1, telemetry_rows=ROWS, **_BOTH)
    assert torch.equal(plain.params, eng.params)
    eng.offset_noise.normal_()  # whatever the buffer holds, the evaluation does not read it
    h, w = H // 8, W // 8
    losses = []
    for e in (plain, eng):
        feed_device_rng(cfg, e, 0, 0, False)
        ph = cfg.clip.vocab_size - 3
        e.set_batch(synth.pixel_values(B, H, W, seed=11), synth.input_ids(B, ph, cfg.clip.vocab_size),
                    torch.full((B,), ph), for_eval=True)
        e.set_noise(synth.gaussian((B, 4, h, w), 13), synth.gaussian((B, 4, h, w), 14), torch.tensor([40, 700]))
        losses.append((e.eval_losses(graph=False), e.eval_losses(graph=True)))
    assert torch.equal(losses[0][0], losses[1][0]) and torch.equal(losses[0][1], losses[1][1])
    assert torch.equal(losses[0][0], losses[0][1]) and float(losses[0][0].min()) > 0
    # ---- the ring row of a training micro-step: plain per-sample MSE of the step's own pred / target.  Host-supplied
    # timesteps (40, 700), so that one sample's weight is not 1
    cfg, eng, _, _, _, _ = build_step("tiny", B, H, W, device_rng=False, lr=4e-3, telemetry_rows=ROWS, **_BOTH)
    inp = _step_inputs(cfg, False, H, W)
    eng.set_batch(inp["px"], inp["ids"], torch.full((B,), cfg.clip.vocab_size - 3))
    eng.set_noise(inp["eps"], inp["noise"], inp["t"], offset_noise=inp["xi"])
    eng.forward_backward()
    Lc, hw = 4, h * w
    direct, ws = torch.zeros(B, device=DEV), torch.zeros_like(eng.eval_ws)
    ops.mse_loss_per_sample(eng.unet.pred, eng.target, direct, ws, B, Lc, hw)
    torch.cuda.synchronize()
    t = eng.timesteps.cpu()
    eng.optimizer_step()
    (row,), lost = eng.read_telemetry()
    assert lost == 0 and row["timesteps"] == t.tolist()
    assert row["losses"] == direct.cpu().tolist(), "the ring's per-sample losses must stay unweighted"
    # loss() is the weighted mean of exactly those
    wts = LR.min_snr_weight(AC, t, GAMMA)
    want = (wts * direct.cpu().double()).mean().item()
    print(f"[weighted loss] t {t.tolist()} w {wts.tolist()} loss() {eng.loss():.6f} weighted mean of the row {want:.6f}")
    assert t.tolist() == list(T_STEP) and float(wts[0]) < 0.5 and float(wts[1]) == 1.0
    assert eng.loss() == pytest.approx(want, rel=1e-5)


@pytest.mark.parametrize("form", ["one-mapper", "mode3"])
def test_launch_counts(form, monkeypatch):
    """an eager step's ABI calls (one kernel launch each for the entries concerned): snr_gamma swaps one entry for the
    other and adds none; noise_offset swaps one and adds one rng_fill_normal; everything else is the plain list in order"""
    from view_neti_amd import lib
    mode3 = FORMS[form][0]

    def calls(**kw):
        cfg, eng = _build(mode3, 1, **kw)
        _feed(cfg, eng, 0, 0, mode3)
        names, orig = [], lib.call
        with monkeypatch.context() as m:
            m.setattr(lib, "call", lambda name, *a: (names.append(name), orig(name, *a))[1])
            assert eng.step()
        torch.cuda.synchronize()
        return names, len(eng.launches())

    plain, n_plain = calls()
    assert "mse_loss_grad_snr" not in plain and "sample_add_noise_offset" not in plain
    snr, n_snr = calls(snr_gamma=GAMMA)
    assert len(snr) == len(plain) and n_snr == n_plain
    assert [n.replace("mse_loss_grad_snr", "mse_loss_grad") for n in snr] == plain and snr.count("mse_loss_grad_snr") == 1
    off, n_off = calls(noise_offset=OFFSET)
    assert len(off) == len(plain) + 1 and n_off == n_plain
    i = off.index("sample_add_noise_offset")
    assert off.count("rng_fill_normal") == plain.count("rng_fill_normal") + 1
    k = [j for j, n in enumerate(off) if n == "rng_fill_normal"][2]   # eps, noise, then the offset draw
    rest = [n for j, n in enumerate(off) if j != k]
    assert k < i and [n.replace("sample_add_noise_offset", "sample_add_noise") for n in rest] == plain
    both, _ = calls(**_BOTH)
    assert len(both) == len(plain) + 1 and "mse_loss_grad" not in both and "sample_add_noise" not in both


# ================================================================================================ Coach
def test_coach_run_with_both_options(tmp_path):
    rt.toys(tmp_path / "toys")
    on = ("--optim.snr_gamma", "5", "--optim.noise_offset", "0.1", "--log.train_metrics", "true")
    cfg = rt.mode0_cfg(tmp_path / "toys", tmp_path / "a", *on, max_steps=3)
    coach = rt.coach(cfg)
    assert coach.engine.snr_gamma == 5.0 and coach.engine.noise_offset == 0.1
    assert rt.train_counting(coach) == 3
    ck = torch.load(cfg.log.exp_dir / "mapper-steps-3_object.pt", map_location="cpu", weights_only=False)
    assert "snr_gamma" not in ck["cfg"]["optim"] and "noise_offset" not in ck["cfg"]["optim"]
    ext = ck["vneti_ext"]["config_ext"]
    assert ext["optim.snr_gamma"] == 5.0 and ext["optim.noise_offset"] == 0.1
    lines = [json.loads(l) for l in (cfg.log.exp_dir / "train-metrics.jsonl").read_text().splitlines()]
    assert [l["step"] for l in lines] == [1, 2, 3]
    for l in lines:
        w = LR.min_snr_weight(AC, [s["t"] for s in l["samples"]], GAMMA)
        want = (w * torch.tensor([s["loss"] for s in l["samples"]], dtype=torch.float64)).mean().item()
        assert l["loss_weighted"] == pytest.approx(want, rel=1e-12) and l["loss_weighted"] <= l["loss"]
        assert l["loss"] == pytest.approx(sum(s["loss"] for s in l["samples"]) / len(l["samples"]), rel=1e-12)
    del coach
    # a run with another gamma, or without one, cannot continue this state: the field is named
    for other in (("--optim.snr_gamma", "4", "--optim.noise_offset", "0.1"), ("--optim.noise_offset", "0.1")):
        cfg2 = rt.mode0_cfg(tmp_path / "toys", tmp_path / f"x{len(other)}", "--model.mapper_checkpoint_path",
                             str(cfg.log.exp_dir / "mapper-steps-3"), *other)
        with pytest.raises(ValueError, match="snr_gamma"):
            rt.coach(cfg2)
