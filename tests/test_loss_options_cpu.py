"""Host side of `optim.snr_gamma` and `optim.noise_offset`: the float64 restatement the GPU tests
compare against (tests/helpers/loss_options_ref.py), the configuration fields, what a checkpoint carries, the resume
fingerprint, and `loss_weighted` in train-metrics.jsonl.  No GPU."""
import json
import math

import pytest
import torch

from helpers import loss_options_ref as LR

from view_neti_amd.compat import config as C
from view_neti_amd.compat import resume as R
from view_neti_amd.compat import train_metrics as TM

AC = LR.scaled_linear_alphas_cumprod_f32()
ALL_T = torch.arange(1000)


# ------------------------------------------------------------------------------------------------ the restatement
def test_table_is_the_engines():
    from view_neti_amd import sd_config as sc
    from view_neti_amd.engine.step import alphas_cumprod
    assert torch.equal(AC, alphas_cumprod(sc.tiny().ddpm))


def test_epsilon_weights():
    gamma = 5.0
    s, w = LR.snr(AC, ALL_T), LR.min_snr_weight(AC, ALL_T, gamma)
    below = s <= gamma
    assert bool((w[below] == 1.0).all())                      # exactly 1 where the SNR is not clipped
    assert torch.allclose(w[~below] * s[~below], torch.full_like(s[~below], gamma), rtol=1e-14, atol=0)  # w snr == gamma
    # SD's scaled-linear schedule: SNR falls with t, from ~1175 at t = 0 to ~0.0047 at t = 999; gamma = 5 cuts at 146 | 147
    assert bool((s[1:] < s[:-1]).all())
    assert s[0].item() == pytest.approx(1175, rel=1e-3) and s[999].item() == pytest.approx(0.0047, rel=1e-2)
    assert s[146].item() == pytest.approx(5.003, abs=5e-4) and s[147].item() == pytest.approx(4.953, abs=5e-4)
    assert int((~below).sum()) == 147 and bool((~below)[:147].all())  # every t <= 146 is down-weighted, no other
    assert w[0].item() == pytest.approx(0.004254, abs=5e-7)
    # gamma = inf: every weight is exactly 1 (snr / snr)
    assert bool((LR.min_snr_weight(AC, ALL_T, math.inf) == 1.0).all())


def test_v_prediction_weights():
    gamma = 5.0
    s, w = LR.snr(AC, ALL_T), LR.min_snr_weight(AC, ALL_T, gamma, v_prediction=True)
    assert torch.equal(w, torch.minimum(s, torch.tensor(gamma, dtype=torch.float64)) / (s + 1.0))
    assert bool((w < 1.0).all()) and bool((w > 0.0).all())
    lo = s <= gamma
    assert torch.allclose(w[lo], s[lo] / (s[lo] + 1.0), rtol=1e-15, atol=0)       # unclipped: snr / (snr + 1) = alphas_cumprod
    assert torch.allclose(w[lo], AC.double()[lo], rtol=1e-12, atol=0)
    assert torch.allclose(w[~lo], gamma / (s[~lo] + 1.0), rtol=1e-15, atol=0)


def test_offset_and_weighted_mse():
    g = torch.Generator().manual_seed(0)
    noise, xi = torch.randn(3, 4, 5, 5, generator=g), torch.randn(3, 4, generator=g)
    n2 = LR.offset_noise(noise, xi, 0.1)
    assert n2.dtype == torch.float64 and torch.equal(LR.offset_noise(noise, xi, 0.0), noise.double())
    d = n2 - noise.double()
    # one value per (sample, channel), s * xi (to the rounding of (n + o) - n in f64)
    assert torch.allclose(d, (0.1 * xi.double())[:, :, None, None].expand_as(d), rtol=0, atol=1e-15)
    # the gradient of the weighted loss is autograd's
    pred = torch.randn(3, 4, 5, 5, generator=g, dtype=torch.float64, requires_grad=True)
    w = LR.min_snr_weight(AC, [0, 146, 147], 5.0)
    loss, grad = LR.weighted_mse(pred, n2, w)
    per_sample = ((pred - n2) ** 2).mean(dim=(1, 2, 3))
    assert loss.item() == pytest.approx((w * per_sample).mean().item(), rel=1e-14)
    loss.backward()
    assert torch.allclose(pred.grad, grad, rtol=1e-13, atol=0)
    # epsilon: the target is the offset noise itself; the noisy latents move by sqrt(1 - a) * the offset
    z = torch.randn(3, 4, 5, 5, generator=g)
    noisy0, _ = LR.add_noise(z, noise, AC, [0, 999, 500], False)
    noisy1, target1 = LR.add_noise(z, n2, AC, [0, 999, 500], False)
    assert torch.equal(target1, n2)
    sb = (1.0 - AC.double()[[0, 999, 500]]).sqrt().view(3, 1, 1, 1)
    assert torch.allclose(noisy1 - noisy0, sb * d, rtol=0, atol=1e-14)


# ------------------------------------------------------------------------------------------------ configuration
ON = ["--optim.snr_gamma", "5", "--optim.noise_offset", "0.1"]


def test_fields_parse_and_validate():
    cfg = C.parse(C.RunConfig, ON)
    assert cfg.optim.snr_gamma == 5.0 and isinstance(cfg.optim.snr_gamma, float) and cfg.optim.noise_offset == 0.1
    plain = C.parse(C.RunConfig, [])
    assert plain.optim.snr_gamma is None and plain.optim.noise_offset is None
    for name in ("snr_gamma", "noise_offset"):
        for bad in ("0", "-1.0", "0.0"):
            with pytest.raises(ValueError, match=name):
                C.parse(C.RunConfig, [f"--optim.{name}", bad])
    # round trip through encode and through the YAML text of config.yaml
    again = C.decode(C.RunConfig, C.encode(cfg))
    assert again.optim.snr_gamma == 5.0 and again.optim.noise_offset == 0.1
    again = C.decode(C.RunConfig, __import__("yaml").safe_load(C.dump(cfg)))
    assert again.optim.snr_gamma == 5.0 and again.optim.noise_offset == 0.1


def test_what_a_checkpoint_and_config_yaml_carry():
    cfg = C.parse(C.RunConfig, ON)
    ckpt_cfg = C.encode(cfg, include_ext=False)
    assert "snr_gamma" not in ckpt_cfg["optim"] and "noise_offset" not in ckpt_cfg["optim"]
    C.decode(C.RunConfig, ckpt_cfg)  # still the reference's schema
    ext = C.ext_fields(cfg)
    assert ext["optim.snr_gamma"] == 5.0 and ext["optim.noise_offset"] == 0.1
    full = C.encode(cfg)
    assert full["optim"]["snr_gamma"] == 5.0 and full["optim"]["noise_offset"] == 0.1
    # each alone: only that one travels
    only = C.parse(C.RunConfig, ["--optim.snr_gamma", "5"])
    assert C.ext_fields(only)["optim.snr_gamma"] == 5.0 and "optim.noise_offset" not in C.ext_fields(only)
    assert "noise_offset" not in C.encode(only)["optim"]
    # a run that uses neither writes the files it always wrote
    plain = C.parse(C.RunConfig, [])
    assert not any("snr_gamma" in k or "noise_offset" in k for k in C.ext_fields(plain))
    assert "snr_gamma" not in C.encode(plain)["optim"] and "noise_offset" not in C.encode(plain)["optim"]


@pytest.mark.parametrize("field", ["snr_gamma", "noise_offset"])
def test_fingerprint_has_the_field_only_when_set(field):
    args = (0, 2, 2, 1, "fp16", 0, 300, 1234)
    unset, on = R.fingerprint(*args), R.fingerprint(*args, **{field: 0.5})
    assert field not in unset and on[field] == 0.5
    assert {k: v for k, v in on.items() if k != field} == unset
    assert unset == {k: v for k, v in R.fingerprint(*args, max_grad_norm=1.0).items() if k != "max_grad_norm"}
    old = dict(unset)  # what a state saved before the field existed holds
    R.check_fingerprint(old, unset)
    R.check_fingerprint(on, on)
    for saved, current in ((old, on), (on, unset), (on, R.fingerprint(*args, **{field: 2.0}))):
        with pytest.raises(ValueError, match=field) as err:
            R.check_fingerprint(saved, current)
        assert "learnable_mode" not in str(err.value)


# ------------------------------------------------------------------------------------------------ train-metrics.jsonl
def _group():
    """a hand-made accumulation group of two micro-steps, B = 2 (the values are exact in f32)"""
    closed = {"skipped": False, "clip_coef": 1.0, "loss_scale": 65536.0, "lr": 0.5,
              "grad_norm": {"object": 3.0, "view": 4.0, "total": 5.0}}
    return [{"micro_step": 0, "micro": 0, "closed": False, "timesteps": [0, 146], "losses": [0.5, 0.25]},
            {"micro_step": 1, "micro": 1, "closed": True, "timesteps": [147, 999], "losses": [2.0, 0.125], **closed}]


def test_loss_weighted_only_when_set():
    plain = TM.step_line(3, _group())
    assert "loss_weighted" not in plain
    assert list(plain) == ["step", "loss", "lr", "loss_scale", "skipped", "grad_norm", "clip_coef", "samples"]
    ac = AC.numpy()
    for vpred in (False, True):
        line = TM.step_line(3, _group(), snr_gamma=5.0, alphas_cumprod=ac, v_prediction=vpred)
        assert list(line) == list(plain) + ["loss_weighted"]
        assert {k: v for k, v in line.items() if k != "loss_weighted"} == plain  # "loss" stays the unweighted mean
        w = LR.min_snr_weight(AC, [0, 146, 147, 999], 5.0, vpred)
        want = (w * torch.tensor([0.5, 0.25, 2.0, 0.125], dtype=torch.float64)).mean().item()
        assert line["loss_weighted"] == pytest.approx(want, rel=1e-14)
        assert json.loads(json.dumps(line, allow_nan=False)) == line
    eps = TM.step_line(3, _group(), snr_gamma=5.0, alphas_cumprod=ac)
    assert eps["loss_weighted"] < plain["loss"]  # t = 0 and 146 are down-weighted, 147 and 999 are not
    assert TM.step_line(3, _group(), snr_gamma=math.inf, alphas_cumprod=ac)["loss_weighted"] == plain["loss"]
    assert [l["loss_weighted"] for l in TM.lines_up_to([_group()], 3, snr_gamma=5.0, alphas_cumprod=ac)] == [eps["loss_weighted"]]
    with pytest.raises(ValueError, match="alphas_cumprod"):
        TM.step_line(3, _group(), snr_gamma=5.0)
    assert TM.min_snr_weight(float(AC[0]), 5.0) == pytest.approx(LR.min_snr_weight(AC, 0, 5.0).item(), rel=1e-15)
