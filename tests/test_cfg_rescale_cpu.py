"""Guidance rescale and trailing timesteps, no GPU: the float64 restatement in tests/helpers/cfg_rescale_ref.py against a
direct torch.std evaluation, `inference_timesteps(..., spacing=)`, the range check of phi, and the new configuration and
command-line fields (all off by default)."""
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from helpers import cfg_rescale_ref as R

from view_neti_amd.compat import config as C
from view_neti_amd.compat import inference_dtu as nvs
from view_neti_amd.engine.infer import check_rescale, inference_timesteps

ROOT = Path(__file__).resolve().parent.parent


@pytest.mark.parametrize("g", [1.0, 7.5])
@pytest.mark.parametrize("phi", [0.3, 0.7, 1.0])
def test_helper_equals_rescale_noise_cfg_written_with_torch_std(g, phi):
    """diffusers' rescale_noise_cfg: std over every non-batch dim (torch.std, unbiased), the guided prediction times
    std_text / std_cfg, blended with weight phi — on a (3, 4, 5, 7) case with an offset and per-sample scales"""
    gen = torch.Generator().manual_seed(5)
    scale = torch.tensor([0.1, 1.0, 10.0], dtype=torch.float64).view(3, 1, 1, 1)
    u = (torch.randn(3, 4, 5, 7, generator=gen, dtype=torch.float64) + 3.0) * scale
    c = (torch.randn(3, 4, 5, 7, generator=gen, dtype=torch.float64) + 3.0) * scale
    e = u + g * (c - u)
    std_c = c.std(dim=[1, 2, 3], keepdim=True)
    std_e = e.std(dim=[1, 2, 3], keepdim=True)
    want_e = phi * (e * (std_c / std_e)) + (1 - phi) * e
    f = R.rescale_factor(u.view(3, 4, 35), c.view(3, 4, 35), g, phi)
    assert f.shape == (3,) and f.dtype == torch.float64
    want_f = (phi * std_c / std_e + (1 - phi)).view(3)
    assert ((f - want_f).abs() / want_f).max().item() < 1e-14
    got_e = f.view(3, 1, 1, 1) * e
    assert ((got_e - want_e).norm() / want_e.norm()).item() < 1e-14
    if g == 1.0:
        assert (f - 1.0).abs().max().item() < 1e-14  # e = c: nothing to rescale
    else:
        assert f.max().item() < 0.9  # guidance inflated the deviation, the factor pulls it back
    # a statistic that is not centred, or shared by the batch, is another number
    rms = phi * (c.pow(2).mean(dim=[1, 2, 3]) / e.pow(2).mean(dim=[1, 2, 3])).sqrt() + (1 - phi)
    shared = phi * c.std() / e.std() + (1 - phi)
    if g != 1.0:
        assert (rms - f).abs().max().item() > 1e-3 and (shared - f).abs().max().item() > 1e-3


def test_helper_constant_prediction_and_float32():
    u = torch.full((2, 4, 9), 0.5, dtype=torch.float64)
    f = R.rescale_factor(u, u.clone(), 7.5, 0.7)
    assert torch.equal(f, torch.ones(2, dtype=torch.float64))  # diffusers: 0 / 0
    gen = torch.Generator().manual_seed(6)
    u, c = torch.randn(2, 4, 64, generator=gen) + 3.0, torch.randn(2, 4, 64, generator=gen) + 3.0
    f32 = R.rescale_factor(u, c, 7.5, 0.7, dtype=torch.float32)
    assert f32.dtype == torch.float32
    assert ((f32.double() - R.rescale_factor(u, c, 7.5, 0.7)).abs().max().item()) < 1e-5
    # the step helper at factor None / ones is the plain step
    x, m, n = (torch.randn(2, 4, 64, generator=gen, dtype=torch.float64) for _ in range(3))
    row = (0.8, 0.6, 0.7, 0.4, -0.2, 0.3)
    e = R.guided(u, c, 7.5)
    for vpred in (False, True):
        a = R.sampler_step(x, e, m, row, n, vpred)
        b = R.sampler_step(x, e, m, row, n, vpred, factor=torch.ones(2))
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        x0 = 0.8 * x - 0.6 * e if vpred else (x - 0.6 * e) / 0.8
        assert torch.allclose(a[1], x0, rtol=1e-15, atol=0)
        assert torch.allclose(a[0], 0.7 * x + 0.4 * x0 - 0.2 * m + 0.3 * n, rtol=1e-14, atol=1e-15)
        assert torch.equal(R.sampler_step(x, e, m, row, None, vpred)[0], 0.7 * x + 0.4 * x0 - 0.2 * m)


def test_trailing_timesteps():
    for kind in ("ddim", "dpm++2m"):
        assert inference_timesteps(kind, 5, spacing="trailing") == [999, 799, 599, 399, 199]
        assert inference_timesteps(kind, 1, spacing="trailing") == [999]
        ts = inference_timesteps(kind, 30, spacing="trailing")
        assert ts[:4] == [999, 966, 932, 899] and ts[-1] == 32 and len(ts) == 30
        for n in (1, 5, 16, 30, 50, 1000):
            ts = inference_timesteps(kind, n, 1000, "trailing")
            assert len(ts) == n and all(isinstance(t, int) for t in ts)
            assert ts == [int(t) for t in np.round(np.arange(1000, 0, -1000 / n)).astype(np.int64) - 1]
            assert all(a > b for a, b in zip(ts, ts[1:])) and 0 <= ts[-1] and ts[0] < 1000
        with pytest.raises(ValueError, match="leading"):
            inference_timesteps(kind, 5, spacing="leading")
        with pytest.raises(ValueError):
            inference_timesteps(kind, 5, spacing="")
    with pytest.raises(ValueError, match="unknown sampler"):
        inference_timesteps("euler", 5, spacing="trailing")


def test_default_spacing_is_the_lists_it_always_gave():
    ddim30 = [958, 925, 892, 859, 826, 793, 760, 727, 694, 661, 628, 595, 562, 529, 496, 463, 430, 397, 364, 331, 298, 265,
              232, 199, 166, 133, 100, 67, 34, 1]
    dpm30 = [999, 966, 932, 899, 866, 832, 799, 766, 733, 699, 666, 633, 599, 566, 533, 499, 466, 433, 400, 366, 333, 300,
             266, 233, 200, 166, 133, 100, 67, 33]
    for kw in ({}, {"spacing": None}):
        assert inference_timesteps("ddim", 5, **kw) == [801, 601, 401, 201, 1]
        assert inference_timesteps("dpm++2m", 5, **kw) == [999, 799, 599, 400, 200]
        assert inference_timesteps("ddim", 30, **kw) == ddim30
        assert inference_timesteps("dpm++2m", 30, **kw) == dpm30
    assert inference_timesteps("ddim", 5, 1000, None) == [801, 601, 401, 201, 1]


def test_phi_range():
    assert check_rescale(0.0) is False and check_rescale(0) is False
    assert check_rescale(0.7) is True and check_rescale(1.0) is True and check_rescale(1e-6) is True
    for bad in (-0.1, 1.0001, 2.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="guidance_rescale"):
            check_rescale(bad)
    with pytest.raises(ValueError, match="guidance_rescale"):
        nvs.InferenceConfig(guidance_rescale=1.5)
    with pytest.raises(ValueError, match="guidance_rescale"):
        C.EvalConfig(guidance_rescale=-0.5)
    with pytest.raises(ValueError, match="timestep_spacing"):
        C.EvalConfig(timestep_spacing="leading")
    with pytest.raises(ValueError, match="timestep_spacing"):
        nvs.InferenceConfig(timestep_spacing="linspace")


def test_sd_pipeline_call_refuses_phi_before_any_draw():
    """the range check comes before the negative prompt, the latents draw and any engine call: a pipeline whose engine
    has nothing but a shape is enough to see it, and the generator is untouched"""
    from types import SimpleNamespace
    from view_neti_amd.compat.sd_pipeline_call import InferencePipeline, sd_pipeline_call
    assert InferencePipeline(None, None).timestep_spacing is None
    assert InferencePipeline(None, None, "ddim", timestep_spacing="trailing").sampler == "ddim"
    pipe = InferencePipeline(SimpleNamespace(B=1, h=8, w=8, Lc=4), None, "ddim")
    gen = torch.Generator().manual_seed(3)
    before = gen.get_state().clone()
    for bad in (1.5, -0.2):
        with pytest.raises(ValueError, match="guidance_rescale"):
            sd_pipeline_call(pipe, torch.zeros(1, 77, 8), guidance_rescale=bad, generator=gen)
    assert torch.equal(gen.get_state(), before)


def test_config_fields_parse_and_default_to_off(tmp_path):
    d = C.parse(C.RunConfig, [])
    assert d.eval.guidance_rescale == 0.0 and d.eval.timestep_spacing is None
    assert not {"guidance_rescale", "timestep_spacing"} & set(C.encode(d)["eval"])
    cfg = C.parse(C.RunConfig, ["--eval.guidance_rescale", "0.7", "--eval.timestep_spacing", "trailing"])
    assert cfg.eval.guidance_rescale == 0.7 and cfg.eval.timestep_spacing == "trailing"
    # run control: the validation's sampler is no part of what a run trained, so neither a checkpoint's cfg nor its
    # extension record (what a resume compares) carries the fields
    assert not {"guidance_rescale", "timestep_spacing"} & set(C.encode(cfg, include_ext=False)["eval"])
    assert not any("guidance_rescale" in k or "timestep_spacing" in k for k in C.ext_fields(cfg))
    assert C.encode(cfg)["eval"]["guidance_rescale"] == 0.7
    with pytest.raises(ValueError, match="guidance_rescale"):
        C.parse(C.RunConfig, ["--eval.guidance_rescale", "1.5"])
    i = nvs.InferenceConfig()
    assert i.guidance_rescale == 0.0 and i.timestep_spacing is None
    i = nvs.parse_inference_config(["--input_dir", str(tmp_path), "--iteration", "10", "--guidance_rescale", "0.7",
                                    "--timestep_spacing", "trailing"])
    assert i.guidance_rescale == 0.7 and i.timestep_spacing == "trailing"
    i = nvs.parse_inference_config(["--input_dir", str(tmp_path), "--iteration", "10"])
    assert i.guidance_rescale == 0.0 and i.timestep_spacing is None


def test_command_lines_take_the_options():
    for script in ("scripts/inference.py", "tools/bench_nvs.py"):
        src = (ROOT / script).read_text()
        assert '"--guidance_rescale"' in src and '"--timestep_spacing"' in src, script
    import inspect
    assert inspect.signature(nvs.generate_views).parameters["guidance_rescale"].default == 0.0
    # the free-prompt command line parses them (argparse stops at the missing --exp_dir otherwise: exit status 2 either way,
    # so look at what it complains about)
    r = subprocess.run([sys.executable, str(ROOT / "scripts" / "inference.py"), "--prompt", "x", "--guidance_rescale", "0.7",
                        "--timestep_spacing", "trailing"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--exp_dir" in r.stderr and "unrecognized" not in r.stderr, r.stderr[-500:]


@pytest.mark.parametrize("precision", ["fp16", "bf16"])
def test_both_libraries_export_the_entries(precision):
    import ctypes
    from view_neti_amd import lib
    names = ["vneti_cfg_rescale_factor", "vneti_cfg_rescale_ws_doubles", "vneti_cfg_sampler_step_scaled",
             "vneti_cfg_sampler_step_scaled_table"]
    assert set(names) <= set(lib.declared_symbols())
    so = ctypes.CDLL(lib.so_path(precision))
    for n in names:
        assert hasattr(so, n), f"{lib.so_path(precision)} lacks {n}"
        assert n[len("vneti_"):] in lib.SIGNATURES
    assert "cfg_rescale_ws_doubles" in lib.VALUE_FUNCS
    # one more operand than the noise entries: const float* factor
    assert len(lib.SIGNATURES["cfg_sampler_step_scaled"]) == len(lib.SIGNATURES["cfg_sampler_step_noise"]) + 1
    assert len(lib.SIGNATURES["cfg_sampler_step_scaled_table"]) == len(lib.SIGNATURES["cfg_sampler_step_noise_table"]) + 1
    so.vneti_cfg_rescale_ws_doubles.restype = ctypes.c_longlong
    # the chunking is fixed by HW alone: the size is linear in Bn; bad shapes answer negative
    one = so.vneti_cfg_rescale_ws_doubles(1, 9216)
    assert one > 0 and one % 4 == 0 and so.vneti_cfg_rescale_ws_doubles(8, 9216) == 8 * one
    assert so.vneti_cfg_rescale_ws_doubles(0, 64) < 0 and so.vneti_cfg_rescale_ws_doubles(1, 0) < 0
