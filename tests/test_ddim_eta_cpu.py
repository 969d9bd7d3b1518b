"""Host algebra of stochastic DDIM (eta > 0), no GPU: `ddim_eta_coefficients` (the six scalars the HIP step kernel reads)
against the float64 restatement of DDIMScheduler.step in tests/helpers/ddim_eta_ref.py, and its eta = 0 row against
`step_coefficients("ddim", ...)`."""

import pytest
import torch

from helpers import ddim_eta_ref as R

from view_neti_amd.engine.infer import check_eta, ddim_eta_coefficients, inference_timesteps, step_coefficients


@pytest.mark.parametrize("vpred", [False, True])
@pytest.mark.parametrize("eta", [0.3, 1.0])
def test_kernel_form_equals_the_scheduler_restatement(eta, vpred):
    """5 DDIM steps on the SD scaled_linear schedule: x <- cx x + c0 x0 + c1 m_prev + cn noise, x0 from (alpha_t, sigma_t),
    equals the scheduler's own update to fp64 round-off (1e-12 relative)"""
    ac = R.scaled_linear_alphas_cumprod()
    steps = 5
    ts = inference_timesteps("ddim", steps)
    assert ts == R.ddim_timesteps(steps) == [801, 601, 401, 201, 1]
    g = torch.Generator().manual_seed(11)
    x = torch.randn(4, 33, generator=g, dtype=torch.float64)
    outs = [torch.randn(4, 33, generator=g, dtype=torch.float64) for _ in ts]
    noise = [torch.randn(4, 33, generator=g, dtype=torch.float64) for _ in ts]
    xk, m_prev, xr = x.clone(), torch.zeros_like(x), x.clone()
    for i, t in enumerate(ts):
        a_t, s_t, cx, c0, c1, cn = ddim_eta_coefficients(ac, ts, i, eta)
        assert c1 == 0.0 and cn > 0.0
        x0 = (a_t * xk - s_t * outs[i]) if vpred else (xk - s_t * outs[i]) / a_t
        xk, m_prev = cx * xk + c0 * x0 + c1 * m_prev + cn * noise[i], x0
        xr, x0r = R.ddim_step(ac, t, t - 1000 // steps, xr, outs[i], eta, noise[i], vpred)
        rel = ((xk - xr).norm() / xr.norm()).item()
        rel0 = ((x0 - x0r).norm() / x0r.norm()).item()
        worst = ((xk - xr).abs() / xr.abs().clamp_min(xr.abs().mean())).max().item()
        print(f"[ddim eta {eta} vpred {vpred} step {i}] x rel {rel:.2e} (worst element {worst:.2e}), x0 rel {rel0:.2e}")
        assert rel < 1e-12 and rel0 < 1e-12 and worst < 1e-12


def test_eta_zero_is_the_deterministic_row():
    ac = R.scaled_linear_alphas_cumprod()
    for steps in (3, 5, 20, 50):
        ts = inference_timesteps("ddim", steps)
        for i in range(steps):
            cx, c0, c1, a_t, s_t = step_coefficients("ddim", ac, ts, i)
            assert ddim_eta_coefficients(ac, ts, i, 0.0) == (a_t, s_t, cx, c0, c1, 0.0)  # exact, and cn == 0


def test_eta_one_last_step_and_variance_shape():
    """the schedule's ends: cn of eta = 1 is the DDPM posterior std, sqrt((1-a_prev)/(1-a_t) (1 - a_t/a_prev)); it scales
    linearly with eta; the last step (prev_t < 0, a_prev = alphas_cumprod[0]) stays finite"""
    ac = R.scaled_linear_alphas_cumprod()
    ts = inference_timesteps("ddim", 5)
    for i, t in enumerate(ts):
        a_t, a_p = ac[t], (ac[t - 200] if t - 200 >= 0 else ac[0])
        want = float(((1 - a_p) / (1 - a_t) * (1 - a_t / a_p)).sqrt())
        row1, row3 = ddim_eta_coefficients(ac, ts, i, 1.0), ddim_eta_coefficients(ac, ts, i, 0.3)
        assert row1[5] == want and abs(row3[5] - 0.3 * want) < 1e-15
        assert all(map(lambda v: v == v and abs(v) < 10, row1))


def test_eta_on_a_sampler_without_one_is_an_error():
    assert check_eta("dpm++2m", 0.0) is False and check_eta("ddim", 0.0) is False and check_eta("ddim", 0.5) is True
    with pytest.raises(ValueError, match="ignores"):
        check_eta("dpm++2m", 0.5)
    with pytest.raises(ValueError):
        check_eta("ddim", -0.1)


@pytest.mark.parametrize("precision", ["fp16", "bf16"])
def test_both_libraries_export_the_noise_step(precision):
    """the header declares the two entries (tests/test_abi.py compares header and exports as sets) and BOTH builds export
    them, with registered ctypes signatures"""
    import ctypes
    from view_neti_amd import lib
    names = ["vneti_cfg_sampler_step_noise", "vneti_cfg_sampler_step_noise_table"]
    assert set(names) <= set(lib.declared_symbols())
    so = ctypes.CDLL(lib.so_path(precision))
    for n in names:
        assert hasattr(so, n), f"{lib.so_path(precision)} lacks {n}"
        assert n[len("vneti_"):] in lib.SIGNATURES
    assert len(lib.SIGNATURES["cfg_sampler_step_noise"]) == 18 and len(lib.SIGNATURES["cfg_sampler_step_noise_table"]) == 14
