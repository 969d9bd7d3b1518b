"""The tests of the norm tests (no GPU): the float64 references of tests/helpers/norm_ref.py against torch's own norms in
double, the proof that the generator's data makes a one-channel group misassignment visible at the WIDEST bar the GPU file
uses (bf16: 8 x 2e-3), the achieved mean / std of the offset-dominated data after rounding to either 16-bit format, and the
numpy emulation of the slab statistics path, which prints what it predicts and asserts nothing about a kernel."""
import pytest
import torch
import torch.nn.functional as F

from helpers import norm_ref as R
from helpers.checks import check, rel

FORMATS = [torch.float16, torch.bfloat16]
BF16_Y_BAR = 2e-3 * 8


@pytest.mark.parametrize("silu", [False, True])
@pytest.mark.parametrize("shape", [(2, 50, 224, 32), (1, 5, 8320, 64), (2, 36, 96, 8)], ids=str)
def test_groupnorm_ref_is_torch_in_double(shape, silu):
    Bn, HW, C, G = shape
    x = R.group_data(Bn, HW, C, G, seed=3).half()
    gamma, beta = R.gn_affine(C)
    dy = torch.randn(Bn, HW, C, generator=torch.Generator().manual_seed(4)).half()
    got = R.groupnorm_ref(x, gamma, beta, G, 1e-5, silu, dy=dy)
    xr = x.double().permute(0, 2, 1).clone().requires_grad_(True)
    yr = F.group_norm(xr, G, gamma.double(), beta.double(), 1e-5)
    yr = F.silu(yr) if silu else yr
    yr.backward(dy.double().permute(0, 2, 1))
    assert rel(got["y"], yr.detach().permute(0, 2, 1)) < 1e-12
    assert rel(got["dx"], xr.grad.permute(0, 2, 1)) < 1e-12
    xg = x.double().reshape(Bn, HW, G, C // G)
    assert rel(got["mean"], xg.mean((1, 3))) < 1e-12
    assert rel(got["rstd"], (xg.var((1, 3), unbiased=False) + 1e-5).rsqrt()) < 1e-12


@pytest.mark.parametrize("rows,C", [(1, 8), (5, 520), (3, 1544)])
def test_layernorm_ref_is_torch_in_double(rows, C):
    g = torch.Generator().manual_seed(5)
    x = (torch.randn(rows, C, generator=g) * 2 + 0.5).half()
    gamma, beta = R.gn_affine(C)
    dy = torch.randn(rows, C, generator=g).half()
    got = R.layernorm_ref(x, gamma, beta, 1e-5, dy=dy)
    xr = x.double().requires_grad_(True)
    yr = F.layer_norm(xr, (C,), gamma.double(), beta.double(), 1e-5)
    yr.backward(dy.double())
    assert rel(got["y"], yr.detach()) < 1e-12
    assert rel(got["dx"], xr.grad) < 1e-12
    assert rel(got["mean"], x.double().mean(-1)) < 1e-12
    assert rel(got["rstd"], (x.double().var(-1, unbiased=False) + 1e-5).rsqrt()) < 1e-12


def test_softmax_ref_is_torch_in_double():
    x = (torch.randn(3, 520, generator=torch.Generator().manual_seed(6)) * 3).half()
    x[0, 0], x[1, -1], x[2, ::3] = 40.0, 40.0, -60000.0
    assert rel(R.softmax_ref(x), torch.softmax(x.double(), -1)) < 1e-12


def test_generator_neighbours_differ():
    """neighbouring groups differ by >= 1 in mean (no ratio) or in the sign of a mean of >= 40 stds (ratio 64)"""
    for Bn, G in [(1, 32), (2, 32), (2, 64), (2, 8)]:
        mean, std = R.group_stats(Bn, G)
        assert ((mean[:, 1:] - mean[:, :-1]).abs() >= 1).all()
        assert (mean.abs() / std).max() <= 4  # benign: no group of the geometry cases is offset-dominated
        mean, std = R.group_stats(Bn, G, ratio=64)
        assert (mean[:, 1:] * mean[:, :-1] < 0).all() and (std == 0.25).all()
        assert len({round(v, 6) for v in mean.abs().flatten().tolist()}) == 3


@pytest.mark.parametrize("dt", FORMATS, ids=["fp16", "bf16"])
@pytest.mark.parametrize("silu", [False, True])
@pytest.mark.parametrize("shape", R.GN_EDGE_SHAPES + [R.GN_RATIO_SHAPE], ids=str)
def test_misassigned_channel_is_visible_at_the_bf16_bar(shape, silu, dt):
    """ONE channel (the last of group 0) normalised with group 1's statistics: `check` refuses it at the bf16 bar, and the
    worst element is at least 10 x over the element-wise allowance — on the data of every GroupNorm case of the GPU file"""
    Bn, HW, C, G = shape
    for ratio in ([None, 64] if shape == R.GN_RATIO_SHAPE else [None]):
        x = R.group_data(Bn, HW, C, G, ratio=ratio, seed=19).to(dt)
        gamma, beta = R.gn_affine(C)
        y = R.groupnorm_ref(x, gamma, beta, G, 1e-5, silu)["y"]
        bad = R.misassign(y, x, gamma, beta, G, 1e-5, silu)
        check("the reference itself", y, y, BF16_Y_BAR)
        excess = R.elem_excess(bad, y, BF16_Y_BAR)
        print(f"{shape} silu{silu} ratio {ratio}: worst element {excess:.1f} x its allowance")
        with pytest.raises(AssertionError):
            check("one misassigned channel", bad, y, BF16_Y_BAR)
        assert excess >= 10, f"{shape} ratio {ratio}: the misassigned channel is only {excess:.2f} x over the allowance"


@pytest.mark.parametrize("dt", FORMATS, ids=["fp16", "bf16"])
def test_ratio_data_keeps_its_ratio_after_rounding(dt):
    Bn, HW, C, G = R.GN_RATIO_SHAPE
    got = R.achieved_ratio(R.group_data(Bn, HW, C, G, ratio=64, seed=19).to(dt), G)
    print(f"{dt}: achieved |mean| / std in [{got.min().item():.1f}, {got.max().item():.1f}]")
    assert got.min() >= 40 and got.max() <= 90


def test_slab_emulation_predictions():
    """the emulation reproduces float64 on benign data (that is all that is asserted, and it is about the emulation); what
    it predicts for offset-dominated groups is printed — a prediction, not a bar"""
    Bn, HW, C, G = 2, 108, 640, 32
    x = R.group_data(Bn, HW, C, G, seed=19).half()
    gamma, beta = R.gn_affine(C)
    ey, em, er = R.slab_prediction(x, gamma, beta, G, 1e-5)
    print(f"benign {(Bn, HW, C, G)}: y {ey:.2e} mean {em:.2e} rstd {er:.2e}")
    assert ey < 1e-5 and em < 1e-6 and er < 1e-5
    Bn, HW, C, G = R.GN_RATIO_SHAPE
    for ratio in R.GN_RATIOS:
        x = R.group_data(Bn, HW, C, G, ratio=ratio, seed=19).half()
        gamma, beta = R.gn_affine(C)
        ey, em, er = R.slab_prediction(x, gamma, beta, G, 1e-5)
        print(f"ratio {ratio} {R.GN_RATIO_SHAPE}: predicted slab-path errors y {ey:.2e} mean {em:.2e} rstd {er:.2e}")
